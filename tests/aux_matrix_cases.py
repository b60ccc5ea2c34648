"""Seeded inputs for every cell of kernel_variants.aux_cells(), and the definitions evaluated on them (no device, no _lib load at
import): what tests/test_aux_matrix_host.py checks the preconditions of on the CPU and tests/test_gpu_aux_matrix.py runs on the device.

Nothing here is new: the model families take kv.scenario's per-member models under saturating random controls (tests/test_gpu_rollout.py),
fc.make_law and gc.weights_and_targets; the fit families the bilinear members of synthetic() (moved here from tests/test_gpu_refit.py,
which imports it back); the online update the random data of tests/test_online_host.py's random_case; the plant families gc.PlantCase
and, for the generator plant, kv.scenario's gen_op0 / gen_ops.  Sizes: B = 5 (one full wavefront of four rows and one more row),
shared and per-member operands where a family has both."""
import functools

import numpy as np

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, fit, online
from oracle import m4q_oracle as orc
from tests import feedback_cases as fc
from tests import grad_cases as gc
from tests import kernel_variants as kv
from tests.test_online_host import ALPHA, two_experiments
from tests.test_refit_host import closed_form, weighted_stacks

B = kv.BATCH
VARIANTS = ("shared", "per")
N_ROLL, N_GRAD, N_FEEDBACK, T_LIN = 7, 6, 8, 6
FIGURES = ("last", "sum")


def _seed(base, nx, nu, order, variant):
    return base + 100 * nx + 10 * nu + order + (1000 if variant == "per" else 0)


def model_sat(p):
    """The configuration's own bound (kv.scenario scales it down for the closed loop): random controls up to it saturate."""
    return p["sat"] / kv.TUNING[(p["dim_x"], p["dim_u"])][1]


# ---------------------------------------------------------------- model families
@functools.lru_cache(maxsize=None)
def model_rollout_case(nx, nu, order, variant):
    """shared: one model, one control sequence, u_scale; per: the members' own models and sequences."""
    p = kv.scenario(nx, nu, order)
    rng = np.random.default_rng(_seed(7800, nx, nu, order, variant))
    sat = model_sat(p)
    c = dict(x0=np.ascontiguousarray(p["x0"]), order=order, sat=sat, m=nu)
    if variant == "per":
        c.update(u=rng.uniform(-sat, sat, (B, N_ROLL, nu)), models=np.ascontiguousarray(p["models"]), u_scale=None)
    else:
        c.update(u=rng.uniform(-sat, sat, (N_ROLL, nu)), models=np.ascontiguousarray(p["models"][0]),
                 u_scale=1 + 0.1 * rng.standard_normal((B, nu)))
    return c


def member_controls(c, b):
    """The controls member b sees, [N, m]."""
    u = c["u"][b] if c["u"].ndim == 3 else c["u"]
    return u if c["u_scale"] is None else c["u_scale"][b] * u


def model_rollout_reference(c):
    """OracleDMDc.predict chained, member by member: [B, N + 1, n]."""
    md = c["models"] if c["models"].ndim == 3 else [c["models"]] * B
    return np.stack([gc.model_chain(md[b], c["m"], c["order"], c["x0"][b], member_controls(c, b)) for b in range(B)])


@functools.lru_cache(maxsize=None)
def model_grad_case(nx, nu, order, variant):
    """shared: one model, one sequence, u_scale, per-member targets; per: the members' own models and sequences, one target."""
    p = kv.scenario(nx, nu, order)
    rng = np.random.default_rng(_seed(9600, nx, nu, order, variant))
    sat = model_sat(p)
    W, f = gc.weights_and_targets(rng, nx, B)
    c = dict(x0=np.ascontiguousarray(p["x0"]), order=order, W=W)
    if variant == "per":
        c.update(u=rng.uniform(-sat, sat, (B, N_GRAD, nu)), models=np.ascontiguousarray(p["models"]), u_scale=None, target=f[0])
    else:
        c.update(u=rng.uniform(-sat, sat, (N_GRAD, nu)), models=np.ascontiguousarray(p["models"][0]),
                 u_scale=1 + 0.1 * rng.standard_normal((B, nu)), target=f)
    return c


def model_grad_reference(c, figure):
    return m4q.model_rollout_grad_reference(c["x0"], c["u"], c["models"], c["order"], c["W"], c["target"], u_scale=c["u_scale"],
                                            figure=figure)


def feedback_noise(rng, hermitian):
    """Per-member sigma (one member noise-free) and a member base beyond 2^32 (tests/test_gpu_feedback.py's _noise)."""
    sigma = 0.03 * rng.uniform(0.5, 1.5, B)
    sigma[0] = 0.0
    return m4q.MeasurementNoise(sigma, 4242, "hermitian" if hermitian else "iid", member_base=(1 << 32) + 17)


@functools.lru_cache(maxsize=None)
def model_feedback_case(nx, nu, order, variant):
    """A law with a band whose bounds bite (fc.make_law), u_scale, a figure, and measurement noise - Hermitian where the state is a
    density matrix, i.i.d. at n = 8.  shared: one law, one model; per: the members' own.  The seed is that of
    tests/test_gpu_feedback.py's test_model_per_step_residuals with its run index 0 (shared) / 1 (per), nothing reseeded."""
    p = kv.scenario(nx, nu, order)
    rng = np.random.default_rng(9600 + 100 * nx + 10 * nu + order + 7 * VARIANTS.index(variant))
    sat = model_sat(p)
    x0 = np.ascontiguousarray(p["x0"])
    models = np.ascontiguousarray(p["models"] if variant == "per" else p["models"][0])
    sc = 1 + 0.1 * rng.standard_normal((B, nu))
    law = fc.make_law(rng, nx, nu, N_FEEDBACK, sat, x0[0], members=B if variant == "per" else None, band=True)
    noise = feedback_noise(rng, nx != 8)
    W, f = gc.weights_and_targets(rng, nx, B)
    return dict(x0=x0, law=law, models=models, order=order, m=nu, kw=dict(u_scale=sc, noise=noise, W=W, target=f, figure="all"))


def model_feedback_define(c, x0=None):
    """The definition's run from x0 (the case's own by default), with the margin of every member to its nearest bound."""
    ref = m4q.model_feedback_reference(c["x0"] if x0 is None else x0, c["law"], c["models"], c["order"], **c["kw"])
    return with_margin(c["law"], ref)


def with_margin(law, ref):
    _, s, lo, hi, _ = fc.law_terms(law, ref["xs"], ref["us"])
    ref["margin"] = np.minimum(np.abs(s - lo), np.abs(s - hi)).min(axis=(1, 2))
    return ref


def feedback_activity(law, ref):
    return fc.activity(law, *fc.law_terms(law, ref["xs"], ref["us"])[:4])


# ---------------------------------------------------------------- fit families
FIT_GRID = np.logspace(-6, -1, 101)
FIT_B, FIT_E, FIT_N = 5, 2, 24
# The plain fit sees the same members without weights, and at (16, 1, 1) the only cut-offs clear of every singular value then lie
# at 1.5e-5 (rank 26 of 32), where the Gram bound is 5e-6: another draw of the same recipe, picked on the CPU from the data's
# singular values alone - the first whose admissible cut-offs include one with a Gram bound under 1e-8 (draws 1 and 2 have no
# admissible cut-off at all)
PLAIN_RESEED = {(16, 1, 1): 3}


def synthetic(n, m, order, prior=True):
    """A case in load_case's form: B bilinear members a few per cent apart under shared weak random controls; the prior of member
    b is the true model of member b + 1.  svals, rank and sens come from NumPy's SVD of the weighted stacks, A from its pinv, and
    the cut-offs are those of 101 points over the training grid's range [1e-6, 1e-1] that are a factor 1.2 clear of every singular
    value of every member: the lowest, the middle one and the highest (the lowest rank).
    prior=False: the same recipe for the plain fit - no prior model, no discount, every snapshot taken (the same data but where
    PLAIN_RESEED draws again)."""
    B, E, N, GRID = FIT_B, FIT_E, FIT_N, FIT_GRID
    rng = np.random.default_rng(1000 * n + 10 * m + order + (0 if prior else 100000 * PLAIN_RESEED.get((n, m, order), 0)))
    P = m4q.size_of_library(order, m) - 1
    nz = n * (1 + P)
    A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    common = np.concatenate([A * (0.9 / np.abs(np.linalg.eigvals(A)).max()),
                             0.3 * (rng.standard_normal((n, n * P)) + 1j * rng.standard_normal((n, n * P))) / np.sqrt(n)], axis=1)
    models = common[None] + 0.03 * (rng.standard_normal((B, n, nz)) + 1j * rng.standard_normal((B, n, nz))) / np.sqrt(n)
    us = (1e-3 if nz == 64 else 1e-2) * rng.uniform(-1, 1, (E, N, m))   # weak: a gap opens between the state and the control block
    xs = np.zeros((B, E, N + 1, n), dtype=complex)
    xs[:, :, 0] = rng.standard_normal((B, E, n)) + 1j * rng.standard_normal((B, E, n))
    pu = fit.lift_controls(us, order)
    for t in range(N):
        z = np.concatenate([xs[:, :, t, None, :], pu[None, :, t, :, None] * xs[:, :, t, None, :]], axis=2).reshape(B, E, nz)
        xs[:, :, t + 1] = np.einsum("bij,bej->bei", models, z)
    if prior:
        c = dict(xs=xs, us=us, order=order, u_scale=None, A0=np.ascontiguousarray(np.roll(models, -1, axis=0)), discount=0.95,
                 counts=np.array([N, N - 5, N, N - 1, N - 9], dtype=np.int32))
    else:
        c = dict(xs=xs, us=us, order=order, u_scale=None, A0=np.zeros((B, n, nz), dtype=complex), discount=1.0,
                 counts=np.full(B, N, dtype=np.int32))
    stacks = [weighted_stacks(c, b) for b in range(B)]
    svals = np.stack([np.concatenate([np.linalg.svd(Z * w, compute_uv=False), np.zeros(max(0, nz - Z.shape[1]))]) for Z, _, w in stacks])
    ok = [rc for rc in GRID if np.all((svals >= 1.2 * rc * svals[:, :1]) | (svals <= rc * svals[:, :1] / 1.2))]
    assert ok, "no cut-off of the grid is clear of every singular value"
    rank = np.stack([(svals > rc * svals[:, :1]).sum(axis=1) for rc in ok])
    pick = sorted({0, len(ok) // 2, len(ok) - 1})
    c.update(rconds=np.array(ok)[pick], rank=rank[pick].astype(np.int32), svals=svals)
    assert (c["rank"] < nz).any(), "no admissible cut-off truncates"
    c["A"] = np.zeros((len(pick), B, n, nz), dtype=complex)
    c["A"] = closed_form(c)
    sens = np.zeros(c["rank"].shape)
    for _ in range(3):                                                         # the rule of tests/test_fit_qr_host.py: three draws
        jit = dict(c, xs=xs * (1 + 1e-15 * rng.standard_normal(xs.shape)), us=us * (1 + 1e-15 * rng.standard_normal(us.shape)))
        sens = np.maximum(sens, np.abs(closed_form(jit) - c["A"]).max(axis=(2, 3)))
    c["sens"] = sens
    return c


@functools.lru_cache(maxsize=None)
def fit_case(nx, nu, order, prior):
    c = synthetic(nx, nu, order, prior)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def fit_args(c, prior):
    """The arguments of dmdc_fit_batch / its two definitions: with the prior (the refit entry points) or the plain call."""
    args = dict(xs=c["xs"], us=c["us"], order=c["order"], rcond=c["rconds"], u_scale=c["u_scale"])
    if prior:
        args.update(A0=c["A0"], discount=c["discount"], counts=c["counts"])
    return args


def fit_members(c, k):
    """The case cut to its first k members (where the definition, a Python loop over rotations, is too slow for all five)."""
    sub = dict(c, **{f: c[f][:k] for f in ("xs", "A0", "counts", "svals")}, **{f: c[f][:, :k] for f in ("rank", "sens", "A")})
    return sub


def fit_definition_members(c):
    """Existing practice (tests/test_gpu_refit.py): the first two members where nz >= 48, else all."""
    return 2 if c["A0"].shape[-1] >= 48 else c["xs"].shape[0]


# ---------------------------------------------------------------- online
ONLINE_N, ONLINE_DISCOUNT = 24, 0.97


@functools.lru_cache(maxsize=None)
def online_case(nx, nu, order):
    """tests/test_online_host.py's random_case at any shape: unit-norm random states, controls in [-1, 1], a random A0 of size 0.1,
    P0 = ALPHA I; N = 24 updates at discount 0.97, E = 1.  The seed is the first for which the definition's sensitivity s stays
    under 1e-11 at every shape in both forms (tests/test_aux_matrix_host.py; worst 2.2e-12): the plain form divides by 1 + z^T P z,
    which nothing keeps away from zero, and with five members one draw in a few comes close."""
    rng = np.random.default_rng([1, nx, nu, order])
    xs = rng.standard_normal((B, 1, ONLINE_N + 1, nx)) + 1j * rng.standard_normal((B, 1, ONLINE_N + 1, nx))
    xs /= np.linalg.norm(xs, axis=-1, keepdims=True)
    nz = kv.lifted_size(nx, nu, order)
    return dict(xs=xs, us=rng.uniform(-1, 1, (ONLINE_N, nu)), order=order, alpha=ALPHA, discount=ONLINE_DISCOUNT, u_scale=None,
                A0=0.1 * (rng.standard_normal((nx, nz)) + 1j * rng.standard_normal((nx, nz))))


def online_args(nx, nu, order, hermitian, E=1):
    c = online_case(nx, nu, order)
    if E == 2:
        c = two_experiments(c)
    return dict(xs=c["xs"], us=c["us"], order=c["order"], A0=c["A0"], alpha=c["alpha"], discount=c["discount"], u_scale=c["u_scale"],
                hermitian=hermitian, hist_every=5, innovations=True)


def online_reference(args):
    return online.online_dmdc_reference(**args)


# ---------------------------------------------------------------- plant families
class GeneratorCase:
    """The generator plant of kv.scenario at (n, m): the Hamiltonian plant's Liouvillian plus amplitude damping.  (16, 2), the
    plant-only shape, has no scenario of its own: config 4's pair under its first two drives, as gc.PlantCase('16-2')."""

    def __init__(self, nx, nu):
        p = kv.scenario(nx, 3 if (nx, nu) == (16, 2) else nu, 1)
        self.kind, self.step = _lib.PLANT_GENERATOR, orc.plant_step_generator
        self.op0, self.ops = np.array(p["gen_op0"][0]), np.array(p["gen_ops"][0][:nu])
        self.dt, self.sat = p["dt"], model_sat(p)
        self.n, self.m, self.d = nx, nu, kv.dd(nx)

    def states(self, rng, count):
        return gc.PlantCase.states(self, rng, count)

    def member_ops(self, rng, count):
        """Per-member generators: the scenario's, with a member's own small Hamiltonian added to the drift and its drives rescaled."""
        op0 = np.stack([self.op0 + m4q.liouvillian(0.1 * gc._herm(rng, self.d)) for _ in range(count)])
        ops = np.stack([(1 + 0.02 * rng.standard_normal()) * self.ops for _ in range(count)])
        return op0, ops


@functools.lru_cache(maxsize=None)
def plant_case(nx, nu, kind):
    if kind == kv.GENERATOR:
        return GeneratorCase(nx, nu)
    return gc.plant_case("%d-%d%s" % (nx, nu, "-process" if kind == kv.PROCESS else ""))


def _plant_seed(base, nx, nu, kind, variant):
    return base + 100 * nx + 10 * nu + kv.PLANT_CODE[kind] - 1 + (1000 if variant == "per" else 0)


def _plant_operands(c, rng, variant, N):
    """shared: one operator set, one control sequence, u_scale, a non-uniform grid; per: the members' own operators and sequences,
    no u_scale, a scalar dt."""
    if variant == "per":
        op0, ops = c.member_ops(rng, B)
        return dict(op0=op0, ops=ops, u=rng.uniform(-c.sat, c.sat, (B, N, c.m)), ts=c.dt, u_scale=None)
    return dict(op0=c.op0, ops=c.ops, u=rng.uniform(-c.sat, c.sat, (N, c.m)), ts=gc.grid(rng, N, c.dt),
                u_scale=1 + 0.1 * rng.standard_normal((B, c.m)))


def dts_of(ts, N):
    return np.full(N, ts) if np.ndim(ts) == 0 else np.diff(ts)


@functools.lru_cache(maxsize=None)
def plant_rollout_case(nx, nu, kind, variant):
    c = plant_case(nx, nu, kind)
    rng = np.random.default_rng(_plant_seed(7000, nx, nu, kind, variant))
    return dict(_plant_operands(c, rng, variant, N_ROLL), c=c, x0=c.states(rng, B))


def plant_rollout_reference(k):
    c = k["c"]
    per = k["op0"].ndim == 3
    dts = dts_of(k["ts"], N_ROLL)
    return np.stack([gc.plant_chain(c, k["x0"][b], member_controls(k, b), k["op0"][b] if per else k["op0"],
                                    k["ops"][b] if per else k["ops"], dts) for b in range(B)])


@functools.lru_cache(maxsize=None)
def plant_grad_case(nx, nu, kind, variant):
    c = plant_case(nx, nu, kind)
    rng = np.random.default_rng(_plant_seed(9500, nx, nu, kind, variant))
    x0 = c.states(rng, B)
    W, f = gc.weights_and_targets(rng, c.n, B)
    return dict(_plant_operands(c, rng, variant, N_GRAD), c=c, x0=x0, W=W, target=f[0] if variant == "per" else f)


def plant_grad_reference(k, figure):
    return m4q.plant_rollout_grad_reference(k["x0"], k["u"], k["op0"], k["ops"], k["ts"], k["W"], k["target"], k["c"].kind,
                                            u_scale=k["u_scale"], figure=figure)


@functools.lru_cache(maxsize=None)
def plant_linearize_case(nx, nu, kind, variant):
    """States that are not Hermitian and controls inside the bound (tests/test_gpu_plant_linearize.py's _points)."""
    c = plant_case(nx, nu, kind)
    rng = np.random.default_rng(_plant_seed(9810, nx, nu, kind, variant))
    X = c.states(rng, B * T_LIN).reshape(B, T_LIN, c.n)
    X = X + 0.05 * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    k = dict(_plant_operands(c, rng, variant, T_LIN), c=c, X=X)
    k["U"] = k.pop("u")
    return k


def plant_linearize_reference(k):
    return m4q.plant_linearize_reference(k["X"], k["U"], k["op0"], k["ops"], k["ts"], k["c"].kind, u_scale=k["u_scale"])


@functools.lru_cache(maxsize=None)
def plant_feedback_case(nx, nu, kind, variant):
    """Per-member operators, a non-uniform grid, u_scale, a law with a band (shared / per member), a figure and measurement noise:
    Hermitian on density matrices, i.i.d. on the process vector."""
    c = plant_case(nx, nu, kind)
    rng = np.random.default_rng(_plant_seed(9700, nx, nu, kind, variant))
    x0 = c.states(rng, B)
    op0, ops = c.member_ops(rng, B)
    ts = gc.grid(rng, N_FEEDBACK, c.dt)
    sc = 1 + 0.1 * rng.standard_normal((B, c.m))
    law = fc.make_law(rng, c.n, c.m, N_FEEDBACK, c.sat, x0[0], members=B if variant == "per" else None, band=True)
    noise = feedback_noise(rng, kind != kv.PROCESS)
    W, f = gc.weights_and_targets(rng, c.n, B)
    return dict(c=c, x0=x0, law=law, op0=op0, ops=ops, ts=ts, kw=dict(u_scale=sc, noise=noise, W=W, target=f, figure="all"))


def plant_feedback_define(k, x0=None):
    ref = m4q.plant_feedback_reference(k["x0"] if x0 is None else x0, k["law"], k["op0"], k["ops"], k["ts"], k["c"].kind, **k["kw"])
    return with_margin(k["law"], ref)

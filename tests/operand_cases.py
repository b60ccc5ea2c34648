"""Operand layouts of the closed loop, for every cell of kernel_variants.closed_loop_cells() (no device, no _lib load).

tests/kernel_variants.py gives every cell one scenario whose target is constant over the window and shared by the members, whose
plant is shared (the process cells aside) and whose models are per member.  mpc_kernel reads a member's target, control target
and plant operators at b * xt_stride, ut_stride, op0_stride, ops_stride, its model at b * model_stride, and chooses between two
instantiations of the backward sweep and of the rollout by whether the target is constant (QP_TARG_CONST; has_tc below).  Two
families of scenarios, derived from kv.scenario / kv.process_scenario at the same sizes (BATCH, HORIZON, STEPS), move what those
scenarios hold still:

"per"     every stride non-zero: per-member CONSTANT targets (kv._spread_states of the scenario's target, columns made with
          np.tile: bit-identical, so a tile cell stays on the tile path), per-member control targets (the scenario's ramp scaled
          and offset per member: u_prev of steps 0 and 1 differs), per-member plant operators (op0 (1 + a b), ops (1 - c b); the
          process cells' Hamiltonians likewise), per-member models as the scenario has them (the process cells share one).
"moving"  every stride zero, the target moving: one shared target X_targ[:, c] = vec(V_c rho V_c^H), V_c = expm(-i theta c G)
          (process cells: the process vector of V_c sigma_x; n = 8: both halves rotated), one shared model (models[0]; the
          shared-generator cells keep their per-member scales: that kernel has no shared-model form), one shared plant.  Members
          differ by x0 alone.  A tile cell opened with such a target must fall back to "traceless".

tests/test_operand_cases_host.py holds the preconditions of every scenario on the CPU; tests/test_gpu_operand_matrix.py runs
them on the device."""
import functools

import numpy as np

from oracle import m4q_oracle as orc
from tests import kernel_variants as kv

PER, MOVING = "per", "moving"
FAMILIES = (PER, MOVING)

# the knobs of the two families.  EPS: the spread of the per-member targets (kv._spread_states); OP0_SPREAD / OPS_SPREAD: a and c of
# the per-member plants; UT_SCALE / UT_OFFSET (in units of sat): member b's control target is U (1 + UT_SCALE b) + UT_OFFSET sat b;
# THETA: the rotation per target column of the moving family (None: the default; per (n, m, order) or (n, m) where the default
# leaves a precondition of tests/test_operand_cases_host.py unmet)
EPS = 0.05
OP0_SPREAD, OPS_SPREAD = 0.03, 0.02
UT_SCALE, UT_OFFSET = 0.1, 0.02
THETA = {None: 0.06, (9, 2): 0.12, (9, 2, 1): 0.2}
# BOX: (sat factor, du factor, further ramp of the control reference in units of sat, R factor) on the scenario's bound, band,
# control reference and control weight, per (n, m, order) or (n, m) (the process cells: "process", m).  kv.TUNING holds the bounds so
# low that the APPLIED controls of the three steps sit on the bound or on the band's edge for most members - which is what the
# variant matrix wants of them, and what would let a wrong target, plant or model go unseen here: us[k] would not move.  These
# factors leave the applied controls of every member inside on some step, and later entries of the guesses on the bound
BOX = {(4, 2): (3.0, 1.0, 3.0, 1.0), (16, 1): (3.0, 1.0, 0.0, 1.0), ("process", 1): (2.0, 4.0, 0.0, 100.0),
       ("process", 3): (2.0, 4.0, 0.0, 60.0)}


def _knob(table, nx, nu, order, process, default):
    keys = [("process", nu, order), ("process", nu)] if process else [(nx, nu, order), (nx, nu)]
    return next((table[k] for k in keys if k in table), default)


def _rebox(p, process):
    fs, fd, ramp, fr = _knob(BOX, p["dim_x"], p["dim_u"], p["order"], process, (1.0, 1.0, 0.0, 1.0))
    p["R"] = fr * np.asarray(p["R"])
    p["sat"] = p["sat"] * fs
    U = np.real(p["U_targ"]) * fs                        # (the control reference ramps in units of sat)
    p["U_targ"] = U + ramp * p["sat"] * np.linspace(0.0, 1.0, U.shape[1])[None, :]
    p["du"] = None if p["du"] is None else p["du"] * fs * fd
    return p


def oracle_plant(cell):
    """The plant the oracle runs for a cell: PLANT_NONE cells take the generator plant's trajectory from the host."""
    return cell.plant if cell.plant in (kv.HAMILTONIAN, kv.PROCESS) else kv.GENERATOR


def expected_path(cell, family):
    """session.path_detail() of the cell under a family: its own, but a tile cell with a moving target runs 'traceless'
    (m4q_capi.hip: supported[PATH_TILE] = traceless && targ_const)."""
    return kv.TRACELESS if (cell.path == kv.TILE and family == MOVING) else cell.path


def only_through_moving(cell):
    """Whether the moving family is what takes this cell off its constant-target code: the general sweep and rollout of a clipped
    kernel that has the tc forms (kv.has_tc), the moving-target branch of the exact kernel's pinned sweep on the real paths
    (pin.tconst), the fall-back of a tile cell."""
    if cell.path == kv.COMPLEX:
        return False
    return cell.path == kv.TILE or cell.exact or kv.has_tc(cell.nx, cell.path)


def _hermitian(rng, d):
    M = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return 0.5 * (M + M.conj().T)


def _base(nx, nu, order, process):
    return kv.process_scenario(nu, order) if process else kv.scenario(nx, nu, order)


def _blocks(nx, process):
    """[(slice of the state vector, d)]: the density matrices a state of the shape holds (n = 8: two side by side)."""
    if process:
        return []
    return [(slice(0, 4), 2), (slice(4, 8), 2)] if nx == 8 else [(slice(0, nx), kv.dd(nx))]


def _unitary_process(V):
    return np.kron(V, V.conj()).reshape(-1)


@functools.lru_cache(maxsize=None)
def scenario(nx, nu, order, process, family, sg=False):
    """The scenario of shape (nx, nu, order) (process: the process plant's) under a family: kv's keys, targets / plant operators
    with a leading member axis where they are per member, and the flags model_per / target_per / plant_per a session is opened
    with.  Cached: callers do not modify it."""
    from scipy.linalg import expm
    p = _rebox(dict(_base(nx, nu, order, process)), process)
    B, n, m, sat = p["batch"], p["dim_x"], p["dim_u"], p["sat"]
    cols = p["X_targ"].shape[1]
    rng = np.random.default_rng(77 + 1000 * nx + 100 * nu + order + (5 if process else 0))
    target = p["X_targ"][:, 0]
    if process:
        # the process scenario's members share x0: give each its own (the first draws of the seed, the same in both families)
        from mpc4quantum_amd.configs import rx
        p["x0"] = np.stack([_unitary_process(rx(1e-3 + 0.05 * rng.standard_normal())) for _ in range(B)])
    if family == PER:
        if process:
            sx = np.array([[0, 1], [1, 0]], dtype=complex)                          # sigma_x: the scenario's gate
            tb = np.stack([_unitary_process(expm(-1j * EPS * _hermitian(rng, 2)) @ sx) for _ in range(B)])
        else:
            tb = np.hstack([kv._spread_states(target[sl].reshape(d, d), d, B, rng, EPS) for sl, d in _blocks(nx, process)])
        p["X_targ"] = np.ascontiguousarray(np.tile(tb[:, :, None], (1, 1, cols)))
        b = np.arange(B)[:, None, None]
        p["U_targ"] = np.real(p["U_targ"])[None] * (1 + UT_SCALE * b) + UT_OFFSET * sat * b
        s0, sk = 1 + OP0_SPREAD * np.arange(B), 1 - OPS_SPREAD * np.arange(B)
        for key0, keyk in (("plant_op0", "plant_ops"), ("gen_op0", "gen_ops")):
            op0, ops = p[key0], p[keyk]
            if op0 is None:                                          # n = 8: the generator plant alone, on the host
                continue
            p[key0] = np.ascontiguousarray(np.broadcast_to(op0, (B,) + op0.shape[1:]) * s0[:, None, None])
            p[keyk] = np.ascontiguousarray(np.broadcast_to(ops, (B,) + ops.shape[1:]) * sk[:, None, None, None])
        p["model_per"], p["target_per"], p["plant_per"] = p["models"].shape[0] > 1, True, True
        return p
    theta = _knob(THETA, nx, nu, order, process, THETA[None])
    X = np.empty((n, cols), dtype=complex)
    if process:
        G = _hermitian(rng, 2)
        sx = np.array([[0, 1], [1, 0]], dtype=complex)
        for c in range(cols):
            X[:, c] = _unitary_process(expm(-1j * theta * c * G) @ sx)
        # one shared plant (a detuned member's)
        p["plant_op0"], p["gen_op0"] = p["plant_op0"][2:3].copy(), p["gen_op0"][2:3].copy()
    else:
        for sl, d in _blocks(nx, process):
            G = _hermitian(rng, d)
            rho = target[sl].reshape(d, d)
            for c in range(cols):
                V = expm(-1j * theta * c * G)
                X[sl, c] = (V @ rho @ V.conj().T).reshape(-1)
    p["X_targ"] = X
    if not sg:
        p["models"] = p["models"][:1].copy()
        p["scales"] = None if p.get("scales") is None else p["scales"][:1].copy()
    p["model_per"], p["target_per"], p["plant_per"] = bool(sg), False, False
    return p


def scenario_of(cell, family):
    return scenario(cell.nx, cell.nu, cell.order, cell.plant == kv.PROCESS, family, family == MOVING and cell.path == kv.SG)


def plant_ops(p, plant):
    """(op0, ops, generator_plant) of the oracle's plant: Hamiltonians, or generators (generator and process plants)."""
    if plant == kv.HAMILTONIAN:
        return p["plant_op0"], p["plant_ops"], False
    return p["gen_op0"], p["gen_ops"], True


def run_oracle(p, plant, exact, trace=None, **over):
    """orc.mpc_batch of scenario p (with the inputs in `over` replaced) under the oracle plant `plant`: (xs, us, codes, solves),
    xs and us time-major as the C ABI holds them."""
    q = dict(p, **over)
    op0, ops, gen = plant_ops(q, plant)
    H = ops if ops.shape[0] > 1 else list(ops[0])
    xs, us, codes, solves = orc.mpc_batch(q["x0"], q["models"], q["dim_u"], q["order"], q["X_targ"], q["U_targ"], q["dt"],
                                          q["horizon"], q["n_steps"], op0, H, q["Q"], q["R"], q["Qf"], q["sat"], q["du"],
                                          qp_mode="exact" if exact else "qp", trace=trace, generator_plant=gen)
    return np.swapaxes(xs, 1, 2), np.swapaxes(us, 1, 2), codes, solves


@functools.lru_cache(maxsize=None)
def _oracle(nx, nu, order, plant, exact, family, sg):
    p = scenario(nx, nu, order, plant == kv.PROCESS, family, sg)
    trace = []
    xs, us, codes, solves = run_oracle(p, plant, exact, trace=trace)
    for a in (xs, us, codes, solves):
        a.setflags(write=False)
    return p, xs, us, codes, solves, trace


def oracle(cell, family, exact=None):
    """(p, xs_t, us_t, codes, solves, trace) of the oracle's run of a cell's scenario under a family (cached: every path of one
    shape and plant shares it; exact: the cell's own solve unless given)."""
    sg = family == MOVING and cell.path == kv.SG
    return _oracle(cell.nx, cell.nu, cell.order, oracle_plant(cell), cell.exact if exact is None else exact, family, sg)


def member(p, b):
    """Member b of a per-member scenario as a B = 1 scenario whose operands are all shared (every stride zero)."""
    q = dict(p, batch=1, x0=p["x0"][b:b + 1].copy(), model_per=False, target_per=False, plant_per=False)
    if p["models"].shape[0] > 1:
        q["models"] = p["models"][b:b + 1].copy()
        if p.get("scales") is not None:
            q["scales"] = p["scales"][b:b + 1].copy()
    if np.ndim(p["X_targ"]) == 3:
        q["X_targ"], q["U_targ"] = p["X_targ"][b].copy(), p["U_targ"][b].copy()
    for key in ("plant_op0", "plant_ops", "gen_op0", "gen_ops"):
        v = p.get(key)
        if v is not None and v.shape[0] > 1:
            q[key] = v[b:b + 1].copy()
    return q


def oracle_keys():
    """Every distinct (nx, nu, order, oracle plant, exact, family, sg) the cells and families above ask the oracle for."""
    keys = []
    for c in kv.closed_loop_cells():
        for family in FAMILIES:
            k = (c.nx, c.nu, c.order, oracle_plant(c), c.exact, family, family == MOVING and c.path == kv.SG)
            if k not in keys:
                keys.append(k)
    return keys


def key_id(k):
    return "%d-%d-%d-%s-%s-%s%s" % (k[0], k[1], k[2], k[3], "exact" if k[4] else "clip", k[5], "-sg" if k[6] else "")


def step_sensitivity(p, plant, exact, b, k, xs_t, us_t, guess):
    """How far the ORACLE's us[k], xs[k + 1] and the guesses it leaves behind move when the SQP guess step k of member b starts
    from is perturbed by a relative 1e-15, -1e-15, 3e-15 (tests/test_gpu_parity.py: _oracle_step_sensitivity):
    (us, xs, x_guess, u_guess), the guesses relative to max(1, |.|) as the GPU tests measure them."""
    q = member(p, b)
    op0, ops, gen = plant_ops(q, plant)
    n = q["dim_x"]
    Am = q["models"][b if q["models"].shape[0] > 1 else 0]
    outs = []
    for eps in (0.0, 1e-15, -1e-15, 3e-15):
        model = orc.OracleDMDc(n, n, Am.shape[1] - n, Am)
        exp = (orc.OracleLExperiment if gen else orc.OracleQExperiment)(op0[0], list(ops[0]))
        clock = orc.OracleClock(q["dt"], q["horizon"], q["n_steps"])
        tr = []
        st = dict(step=k, xs=xs_t[b].T, us=us_t[b].T, X_guess=guess[0] * (1 + eps), U_guess=guess[1])
        (x2, u2), _, _ = orc.mpc(q["x0"][0], q["dim_u"], q["order"], q["X_targ"], q["U_targ"], clock, exp, model, q["Q"], q["R"],
                                 q["Qf"], sat=q["sat"], du=q["du"], start=st, stop=k + 1, trace=tr,
                                 qp_mode="exact" if exact else "qp")
        outs.append((u2[:, k], x2[:, k + 1], tr[-1][0], tr[-1][1]))
    ref = outs[0]
    scale = [1.0, 1.0, max(1.0, np.abs(ref[2]).max()), max(1.0, np.abs(ref[3]).max())]
    return tuple(max(np.abs(o[i] - ref[i]).max() for o in outs[1:]) / scale[i] for i in range(4))

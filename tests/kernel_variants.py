"""Every compiled kernel variant of the library, enumerated on the host (no device, no _lib load).

The shapes come from csrc/m4q_shapes.inc through build.py's shapes(); which mpc_kernel<S, PLANT, EXACT, TL, TILE, SG> instances one
shape's object holds follows the rules of m4q_kernels.hip (SQUARE, QUARTIC, HAS_TILE, HAS_SG, pick_kernel / pick_plant), mirrored
below, and which objects go into libm4q_hip_gen.so follows build.py.  tests/test_kernel_variants_host.py pins the rule lines of
both files to the text these mirrors were written against, so a new shape or a changed rule changes the matrix or fails there.

closed_loop_cells() is what tests/test_gpu_variant_matrix.py runs one teacher-forced case of each; entry_point_cells() lists the
single-kernel entry points (linearize, quad_program, discretize, plant_step) per shape; aux_cells() lists every instance of the
auxiliary kernel families (rollouts, gradients, feedback laws, plant linearisation, the four fits, the online update) from mirrors
of M4Q_NO_AUX, FitLayout / OnlineLayout and the plant dispatch: what tests/test_gpu_aux_matrix.py runs one case of each.
param_cells() lists every plant_param_grad_kernel<PLANT, PT> (tests/test_plant_param_host.py pins its rule lines,
tests/test_gpu_plant_param.py runs every one).
scenario() gives seeded, well-conditioned host inputs for every closed-loop shape in the configs.build dict layout.  pieces() mirrors how one launch cuts a member's run into
work items (tests/test_gpu_launch_schedule.py); _planned() / _check_planned() plan exits on a member's own stored states and check
them (tests/test_gpu_exit_condition.py, tests/test_gpu_launch_schedule.py)."""
import importlib.util
import itertools
import os
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc4quantum_amd", "csrc")

# session.path_detail() names of the arithmetic paths (m4q_args.h, enum Path: PATH_COMPLEX .. PATH_SG = 0 .. 4)
COMPLEX, REAL, TRACELESS, TILE, SG = "complex", "real", "traceless", "traceless-tile", "traceless-sg"
# plant kinds (include/m4q.h, _lib.PLANT_*)
NONE, HAMILTONIAN, GENERATOR, PROCESS = "none", "hamiltonian", "generator", "process"
PLANT_CODE = {NONE: 0, HAMILTONIAN: 1, GENERATOR: 2, PROCESS: 3}

# the case sizes of every closed-loop cell: one full wavefront of four rows and one more row; a horizon that is not a multiple of
# the tile sweep's four and spans two of its blocks; three MPC steps (two of them warm: the line search, then the full step)
BATCH, HORIZON, STEPS = 5, 7, 3
# the run of tests/test_gpu_launch_schedule.py: past the last cut of the exact kernel (XCUTS), so that one launch makes every piece
LONG_STEPS = 14
XCUTS = (4, 7, 12)


# ---------------------------------------------------------------- rule mirrors (m4q_kernels.hip, build.py)
def shapes():
    """[(nx, nu, order, plant_only)] as build.py reads m4q_shapes.inc."""
    spec = importlib.util.spec_from_file_location("m4q_csrc_build", os.path.join(CSRC, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    return build.shapes()


def dd(nx):
    """constexpr int DD = (NX == 4) ? 2 : (NX == 9) ? 3 : (NX == 16) ? 4 : 1;"""
    return {4: 2, 9: 3, 16: 4}.get(nx, 1)


def fourth_root(n):
    """m4q_mpc.h fourth_root: d with d^4 = n, 0 if there is none."""
    d = 1
    while d ** 4 <= n:
        if d ** 4 == n:
            return d
        d += 1
    return 0


def square(nx):
    return dd(nx) * dd(nx) == nx


def quartic(nx):
    return fourth_root(nx) > 0


def has_tile(nx, order):
    return square(nx) and order == 1 and nx - 1 <= 8


def has_sg(nx, order):
    return square(nx) and order == 1 and nx == 16


def has_gen_object(nx, plant_only):
    """build.py: a kernelsg_* object (libm4q_hip_gen.so) for d = {4: 2, 9: 3, 16: 4}.get(nx) and not plant_only."""
    return {4: 2, 9: 3, 16: 4}.get(nx) is not None and not plant_only


def clipped_paths(nx, order):
    """pick_kernel, clipped solve: !SQUARE builds the complex kernel alone; path 4 where HAS_SG, path 3 where HAS_TILE."""
    if not square(nx):
        return [COMPLEX]
    return [COMPLEX, REAL, TRACELESS] + ([TILE] if has_tile(nx, order) else []) + ([SG] if has_sg(nx, order) else [])


def exact_paths(nx, order):
    """pick_kernel, exact solve: path 4 falls back to 2 (no sg exact kernel); path 3 is the one exact traceless kernel with its
    pinned sweep on tiles (exact_tile: EXACT && TL && HAS_TILE)."""
    if not square(nx):
        return [COMPLEX]
    return [COMPLEX, REAL, TRACELESS] + ([TILE] if has_tile(nx, order) else [])


TC_MIN_N = 8                             # constexpr int TC_MIN_N = 8;


def n_state(nx, path):
    """NS, the dimension of a kernel's recursion: nx - 1 on the traceless coordinates (coords_of: paths 2, 3, 4), else nx."""
    return nx - 1 if path in (TRACELESS, TILE, SG) else nx


def has_tc(nx, path):
    """constexpr bool HAS_TC = NS >= TC_MIN_N && sizeof(S) == sizeof(double);  (mpc_kernel, the clipped solve off the tiles): the
    kernel holds a constant-target instantiation of the backward sweep and of the rollout (riccati_backward<.., false, true>,
    rollout_forward<.., false, true>, rollout_forward_pair at NS = 8) beside the general one and picks by QP_TARG_CONST at run
    time.  S is double on every path but the complex one."""
    return path not in (COMPLEX, TILE) and n_state(nx, path) >= TC_MIN_N


def pieces(step_begin, step_end, exact):
    """The work items [begin, end) mpc_kernel makes of one member's run [step_begin, step_end): two_phase (step_begin < 2 and
    step_end > 2) cuts a head [step_begin, 2) off the rest, and the exact kernel cuts the rest again at every XCUTS[i] below
    step_end (n_pieces); piece i >= 1 begins at piece_cut(i): 2, XCUTS[0], XCUTS[1], ..."""
    two_phase = step_begin < 2 and step_end > 2
    n = 2 if two_phase else 1
    if exact:
        n += sum(1 for c in XCUTS if two_phase and step_end > c)
    cut = (2,) + XCUTS
    return [(step_begin if i == 0 else cut[i - 1], step_end if i == n - 1 else cut[i]) for i in range(n)]


def plants(nx, path, plant_only=False):
    """pick_plant: !SQUARE runs PLANT_NONE alone; the generator plant lives in the gen object; the process plant is built for
    QUARTIC shapes on the complex kernel only (S = cplx, !TL, !TILE, !SG)."""
    if not square(nx):
        return [NONE]
    out = [NONE, HAMILTONIAN]
    if has_gen_object(nx, plant_only):
        out.append(GENERATOR)
    if quartic(nx) and path == COMPLEX:
        out.append(PROCESS)
    return out


# ---------------------------------------------------------------- the cells
LoopCell = namedtuple("LoopCell", "nx nu order path exact plant")
EntryCell = namedtuple("EntryCell", "kind nx nu order mode")


def cell_id(c):
    if isinstance(c, LoopCell):
        return "%d-%d-%d-%s-%s-%s" % (c.nx, c.nu, c.order, c.path, "exact" if c.exact else "clip", c.plant)
    return "%s-%d-%d-%d-%s" % (c.kind, c.nx, c.nu, c.order, c.mode)


def closed_loop_cells():
    cells = []
    for nx, nu, order, plant_only in shapes():
        if plant_only:
            continue
        for exact, paths in ((False, clipped_paths(nx, order)), (True, exact_paths(nx, order))):
            for path in paths:
                for plant in plants(nx, path, plant_only):
                    cells.append(LoopCell(nx, nu, order, path, exact, plant))
    return cells


QP_MODES = ("qp", "ref_lqr", "du_band", "exact")


def entry_point_cells():
    """linearize per closed-loop shape; quad_program per distinct (n, m) in every mode; discretize per shape at orders 1-2;
    plant_step per (n, m) with a device plant (square n, plant-only shapes included), Hamiltonian and generator."""
    sh = shapes()
    cells = [EntryCell("linearize", nx, nu, o, "-") for nx, nu, o, po in sh if not po]
    nm = sorted({(nx, nu) for nx, nu, o, po in sh if not po})
    cells += [EntryCell("qp", nx, nu, 0, mode) for (nx, nu), mode in itertools.product(nm, QP_MODES)]
    cells += [EntryCell("discretize", nx, nu, o, "-") for nx, nu, o, po in sh if not po and o <= 2]
    pm = sorted({(nx, nu) for nx, nu, o, po in sh if square(nx)})
    cells += [EntryCell("plant", nx, nu, 0, kind) for (nx, nu), kind in itertools.product(pm, (HAMILTONIAN, GENERATOR))]
    return cells


# ---------------------------------------------------------------- the auxiliary families
# (rollouts, gradients, stored feedback laws, plant linearisation, the four DMDc fits, the online update)
REFUSED = "refused"                      # the kind of a cell whose entry point refuses the shape or plant before any launch
PLAIN, HERMITIAN_FORM = "plain", "hermitian-form"                     # online_dmdc_kernel<.., HERM>: HERM = false, true
MODEL_FAMILIES = ("model_rollout", "model_grad", "model_feedback")
FIT_FAMILIES = ("fit", "fit_qr", "refit", "refit_qr")
PLANT_FAMILIES = ("plant_rollout", "plant_feedback", "plant_grad", "plant_linearize")
FIT_LDS_LIMIT = 160 * 1024
AUX_GRID = 4096                          # every auxiliary launch caps its grid here and loops
ROWS = 4                                 # members per wavefront of a quad kernel (m4q_mpc.h)
QUAD_WRAP = AUX_GRID * ROWS              # grid_for: a quad kernel takes its second trip from this member on


def n_lifted(nu, order):
    """PowTab<NU, ORDER>::NP: the monomials of degree 1 .. order in nu controls, C(nu + order, order) - 1."""
    from math import comb
    return comb(nu + order, order) - 1


def lifted_size(nx, nu, order):
    """static constexpr int NZ = NX * (1 + PowTab<NU, ORDER>::NP);"""
    return nx * (1 + n_lifted(nu, order))


def fit_lds_bytes(nx, nu, order):
    """FitLayout: G = 0, V = G + NZ * PITCH, C = V + NZ * PITCH, Z = C + NX * PITCH, XN = Z + NZ, LAM = XN + NX;
    ELEMS = LAM + (NZ + 1) / 2; BYTES = sizeof(cplx) * ELEMS."""
    nz = lifted_size(nx, nu, order)
    pitch = nz | 1
    lam = 2 * nz * pitch + nx * pitch + nz + nx
    return 16 * (lam + (nz + 1) // 2)


def online_lds_bytes(nx, nu, order):
    """OnlineLayout: P = 0, A = P + NZ * PITCH, Z = A + NX * PITCH, XN = Z + NZ, PZ = XN + NX, W = PZ + NZ, R = W + NZ, GR = R + NX;
    ELEMS = GR + NX; BYTES = sizeof(cplx) * ELEMS."""
    nz = lifted_size(nx, nu, order)
    pitch = nz | 1
    gr = nz * pitch + nx * pitch + nz + nx + nz + nz + nx
    return 16 * (gr + nx)


def fit_fits(nx, nu, order):
    """static constexpr bool FITS = NZ <= 64 && BYTES <= FIT_LDS_LIMIT;  (FitLayout)"""
    return lifted_size(nx, nu, order) <= 64 and fit_lds_bytes(nx, nu, order) <= FIT_LDS_LIMIT


def online_fits(nx, nu, order):
    """static constexpr bool FITS = NZ <= 64 && BYTES <= FIT_LDS_LIMIT;  (OnlineLayout)"""
    return lifted_size(nx, nu, order) <= 64 and online_lds_bytes(nx, nu, order) <= FIT_LDS_LIMIT


def plant_kinds(nx):
    """launch_by_plant / launch_plant_feedback: nothing where !SQUARE; the Hamiltonian plant, the process plant where QUARTIC, and
    the generator plant otherwise.  (These kernels live in the shape's own object - the plant-only one included -, not in the gen
    object, which holds closed-loop kernels alone: M4Q_NO_AUX.)"""
    if not square(nx):
        return []
    return [HAMILTONIAN, GENERATOR] + ([PROCESS] if quartic(nx) else [])


AuxCell = namedtuple("AuxCell", "family nx nu order kind")


def aux_cell_id(c):
    return "%s-%d-%d-%d-%s" % c


def aux_cells():
    """Every auxiliary kernel instance the library holds, and every (shape, plant) an auxiliary entry point refuses by rule: the
    list of record of what tests/test_gpu_aux_matrix.py runs.  Model-side families per (nx, nu, order) object built without
    M4Q_NO_AUX; fit and online families where their layout FITS, a REFUSED cell where it does not; plant families per (nx, nu) -
    find_shape_any_order picks one object for all orders, plant-only shapes included - and plant kind, order 0, with the generator
    plant REFUSED by the gradient and linearisation entry points."""
    sh = shapes()
    cells = []
    for nx, nu, order, plant_only in sh:
        if plant_only:                                          # M4Q_PLANT_ONLY defines M4Q_NO_AUX: the plant families alone
            continue
        cells += [AuxCell(f, nx, nu, order, "-") for f in MODEL_FAMILIES]
        cells += [AuxCell(f, nx, nu, order, "-" if fit_fits(nx, nu, order) else REFUSED) for f in FIT_FAMILIES]
        if online_fits(nx, nu, order):
            cells += [AuxCell("online", nx, nu, order, form) for form in (PLAIN, HERMITIAN_FORM)]
        else:
            cells.append(AuxCell("online", nx, nu, order, REFUSED))
    for nx, nu in sorted({(nx, nu) for nx, nu, o, po in sh if square(nx)}):
        for kind in plant_kinds(nx):
            cells += [AuxCell(f, nx, nu, 0, kind) for f in ("plant_rollout", "plant_feedback")]
            cells += [AuxCell(f, nx, nu, 0, REFUSED if kind == GENERATOR else kind) for f in ("plant_grad", "plant_linearize")]
    return cells


def param_dim(nx, kind):
    """constexpr int D = PLANT == PLANT_PROCESS ? DQ : DD;  (launch_param_pt, plant_param_grad_kernel)"""
    return fourth_root(nx) if kind == PROCESS else dd(nx)


def param_cells():
    """[(nx, nu, kind, PT)]: every plant_param_grad_kernel<PLANT, PT> the library holds.  The kernel lives in the order-1 object of
    every square shape that is not plant-only (#if !defined(M4Q_NO_AUX) && M4Q_ORDER == 1), for the Hamiltonian plant and, where
    QUARTIC, the process plant (launch_param_by_plant), and launch_param_pt counts PT up from 1 while (1 + PT) * D <= 16."""
    nm = sorted({(nx, nu) for nx, nu, o, po in shapes() if square(nx) and not po and o == 1})
    cells = []
    for kind in (HAMILTONIAN, PROCESS):
        for nx, nu in nm:
            if kind == PROCESS and not quartic(nx):
                continue
            cells += [(nx, nu, kind, pt) for pt in range(1, 16 // param_dim(nx, kind))]
    return cells


def param_waves(nx, kind, pt):
    """constexpr int param_waves() { return (1 + PT) * (PLANT == PLANT_PROCESS ? DQ : DD) > 6 ? 1 : WAVES; }
    constexpr int WAVES = NX <= 9 ? 2 : 1;"""
    return 1 if (1 + pt) * param_dim(nx, kind) > 6 else (2 if nx <= 9 else 1)


# ---------------------------------------------------------------- scenarios
def _spread_states(rho, d, B, rng, eps=0.05):
    """B distinct density matrices near rho: exp(-i eps H_b) rho exp(i eps H_b) with seeded Hermitian H_b."""
    from scipy.linalg import expm
    out = []
    for _ in range(B):
        M = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
        V = expm(-0.5j * eps * (M + M.conj().T))
        out.append((V @ rho @ V.conj().T).reshape(-1))
    return np.ascontiguousarray(out)


def lindblad(c):
    """Dissipator of a collapse operator c on vec_r(rho) (row-major): c rho c^H - {c^H c, rho} / 2."""
    d = c.shape[0]
    cd = c.conj().T
    eye = np.eye(d)
    return np.kron(c, c.conj()) - 0.5 * (np.kron(cd @ c, eye) + np.kron(eye, (cd @ c).T))


def _finish(p, rng, drive_spread=0.05):
    """Per-member models from the scenario's generators: every member gets its own drive scales (and keeps any drift scale the
    configuration draws), and the generator plant of the scenario (the Hamiltonian plant's Liouvillian plus amplitude damping)."""
    from mpc4quantum_amd.vectorize import discretize_homogeneous, liouvillian
    B, m, d = p["batch"], p["dim_u"], p["d"]
    sc = np.ones((B, 1 + m)) if p.get("scales") is None else np.array(p["scales"], dtype=float)
    sc[:, 1:] *= 1 + drive_spread * rng.standard_normal((B, m))
    p["scales"] = sc
    p["models"] = np.ascontiguousarray(discretize_homogeneous([sc[:, k, None, None] * p["generators"][k][None] for k in range(1 + m)],
                                                              p["dt"], p["order"]))
    if square(p["dim_x"]):
        a = np.diag(np.sqrt(np.arange(1, d)), 1).astype(complex)       # lowering operator of the d levels
        p["gen_op0"] = (liouvillian(p["plant_op0"][0]) + 0.02 * lindblad(a))[None]
        p["gen_ops"] = np.stack([liouvillian(h) for h in p["plant_ops"][0]])[None]
    return p


# (R scale, sat scale, control-reference ramp in units of sat) per (n, m): R large enough that the SQP steps are well conditioned
# (a handful of line-search iterations on the cold steps), sat low enough that bounds are active in every scenario, and where one
# bound-saturated stretch at the start of the horizon would leave the clipped rollout optimal (one drive; the reduced pair), a
# control reference that ramps past sat over the window, so that LATE controls saturate and the exact solve differs from clipping
TUNING = {(4, 1): (1000.0, 1.0, 3.0), (4, 2): (1000.0, 0.03, 0.0), (9, 2): (1000.0, 0.3, 0.0), (16, 3): (1000.0, 1.0, 0.0),
          (16, 1): (1000.0, 1.0, 3.0), (8, 2): (1000.0, 1.0, 3.0), "process": (3.0, 0.21, 4.3)}


def _tune(p, key):
    r, s, ramp = TUNING[key]
    p["R"] = r * np.asarray(p["R"])
    p["sat"] = s * p["sat"]
    p["du"] = None if p["du"] is None else s * p["du"]
    U = np.zeros_like(np.real(p["U_targ"])) if key == "process" else np.real(p["U_targ"])
    p["U_targ"] = U + ramp * p["sat"] * np.linspace(0.0, 1.0, U.shape[1])[None, :]
    return p


def _targets(target, m, ns, T):
    return np.tile(np.reshape(target, (-1, 1)), (1, ns + T + 1)), np.zeros((m, ns + T))


def scenario(nx, nu, order, batch=BATCH, horizon=HORIZON, n_steps=STEPS):
    """Seeded host inputs of the closed loop at shape (nx, nu, order): the keys of configs.build, with per-member models [B, n,
    n(1+P)] built by discretize_homogeneous from `generators` and `scales` [B, 1+m], distinct per-member initial states, and
    (square n) `gen_op0` [1, n, n] / `gen_ops` [1, m, n, n]: the generator plant."""
    from mpc4quantum_amd import configs
    from mpc4quantum_amd.configs import I2, SX, SY, SZ, rx
    from mpc4quantum_amd.vectorize import liouvillian
    rng = np.random.default_rng(1000 * nx + 100 * nu + order)
    kw = dict(batch=batch, order=order, horizon=horizon, n_steps=n_steps)
    key = (nx, nu)
    if key == (4, 1):
        # config 1: the detuned qubit driven from |0> to |1>
        p = configs.build(1, **kw)
        p["x0"] = _spread_states(p["x0"][0].reshape(2, 2), 2, batch, rng)
    elif key == (4, 2):
        # test_closed_loop_qubit_with_two_quadrature_drives: sigma_x and sigma_y drives towards |+i><+i|
        dt, sat = 0.5, 2 * np.pi * 0.08
        H0, Hk = 0.15 * SZ, [0.5 * SX, 0.5 * SY]
        r0 = rx(0.3)
        X, U = _targets(np.array([0.5, -0.5j, 0.5j, 0.5]), 2, n_steps, horizon)
        p = dict(name="qubit2q", dim_x=4, dim_u=2, d=2, order=order, dt=dt, horizon=horizon, n_steps=n_steps, sat=sat, du=0.5 * sat,
                 Q=np.eye(4), R=1e-2 / sat ** 2 * np.eye(2), Qf=np.eye(4),
                 x0=_spread_states(r0 @ np.diag([1.0, 0]).astype(complex) @ r0.conj().T, 2, batch, rng),
                 generators=np.stack([liouvillian(H0)] + [liouvillian(h) for h in Hk]), scales=None, X_targ=X, U_targ=U,
                 plant_op0=H0[None], plant_ops=np.stack(Hk)[None], batch=batch)
    elif key == (9, 2):
        # config 3: the DRAG transmon, drift scale per member
        p = configs.build(3, **kw)
        p["x0"] = _spread_states(p["x0"][0].reshape(3, 3), 3, batch, rng)
    elif key == (16, 3):
        # config 4: two coupled qubits, coupling J per member
        p = configs.build(4, **kw)
        p["x0"] = _spread_states(p["x0"][0].reshape(4, 4), 4, batch, rng)
    elif key == (16, 1):
        # config 4's drift and its first drive alone (sigma_y on qubit 1): flip qubit 1 of the pair - a d = 4 density matrix
        # under one drive, the shape gate synthesis added, on its Hamiltonian path
        c4 = configs.build(4, batch=batch, horizon=horizon, n_steps=n_steps)
        H0, H1 = np.kron(SZ, SZ), np.kron(SY, I2)
        p0, p1 = np.diag([1.0, 0]).astype(complex), np.diag([0, 1.0]).astype(complex)
        X, U = _targets(np.kron(p1, p0).reshape(-1), 1, n_steps, horizon)
        p = dict(name="pair1drive", dim_x=16, dim_u=1, d=4, order=order, dt=c4["dt"], horizon=horizon, n_steps=n_steps,
                 sat=c4["sat"], du=c4["du"], Q=c4["Q"], R=1e-3 * np.eye(1), Qf=c4["Qf"], x0=c4["x0"],
                 generators=np.stack([liouvillian(H0), liouvillian(H1)]), scales=c4["scales"][:, :2].copy(), X_targ=X, U_targ=U,
                 plant_op0=H0[None], plant_ops=H1[None, None], batch=batch)
        p["x0"] = _spread_states(p["x0"][0].reshape(4, 4), 4, batch, rng)
    elif key == (8, 2):
        # the reduced crosstalk model (test_mpc_crosstalk_model_on_reduced_states): two qubit states side by side, block diagonal;
        # no device plant at n = 8 - the host supplies the states, here from the model's own generators with a small detuning
        z = np.zeros((4, 4))
        L1 = [liouvillian(0 * SX), liouvillian(SX)]
        L2 = [liouvillian(0 * SY), liouvillian(SY)]
        gens = np.stack([np.block([[L1[0], z], [z, L2[0]]]), np.block([[L1[1], z], [z, z]]), np.block([[z, z], [z, L2[1]]])])
        sat = 2 * np.pi * 0.1
        r1, r2 = rx(1e-2), rx(-1e-2)
        p0, p1 = np.diag([1.0, 0]).astype(complex), np.diag([0, 1.0]).astype(complex)
        a = _spread_states(r1 @ p0 @ r1.conj().T, 2, batch, rng)
        b = _spread_states(r2 @ p0 @ r2.conj().T, 2, batch, rng)
        X, U = _targets(np.hstack([p1.reshape(-1), p1.reshape(-1)]), 2, n_steps, horizon)
        det = np.block([[liouvillian(0.05 * SZ), z], [z, liouvillian(-0.05 * SZ)]])
        p = dict(name="crosstalk_reduced", dim_x=8, dim_u=2, d=0, order=order, dt=0.5, horizon=horizon, n_steps=n_steps, sat=sat,
                 du=0.5 * sat, Q=np.diag([1.0, 0, 0, 1, 1, 0, 0, 1]), R=1e-2 / sat ** 2 * np.eye(2),
                 Qf=np.diag([1.0, 0, 0, 1, 1, 0, 0, 1]), x0=np.ascontiguousarray(np.hstack([a, b])), generators=gens, scales=None,
                 X_targ=X, U_targ=U, plant_op0=None, plant_ops=None, batch=batch,
                 gen_op0=(gens[0] + det)[None], gen_ops=gens[1:][None])
    else:
        raise KeyError("no scenario for shape (%d, %d, %d): add one to tests/kernel_variants.py" % (nx, nu, order))
    p["dim_x"], p["dim_u"], p["order"] = nx, nu, order
    return _finish(_tune(p, key), rng)


def process_scenario(nu, order, batch=BATCH, horizon=HORIZON, n_steps=STEPS):
    """The process plant's cells (16, nu, order): configs.synthesis (the NOT gate on the process vector of one qubit) with
    detuned members - driven by sigma_x / 2 alone (nu = 1) or by sigma_x / 2, sigma_y / 2, sigma_z / 2 (nu = 3) - and the
    generators of the same plant on P for the oracle (-i (H (x) I - I (x) H^*) (x) I_4 on vec_r of the 4 x 4 process matrix)."""
    from mpc4quantum_amd import configs
    from mpc4quantum_amd.configs import SX, SY, SZ
    from mpc4quantum_amd.vectorize import discretize_homogeneous
    p = configs.synthesis(batch, order, detuning_spread=0.3, horizon=horizon, n_steps=n_steps)
    eye = np.identity(2)

    def gen(h):
        return np.kron(-1j * (np.kron(h, eye) - np.kron(eye, h.conj())), np.identity(4))
    if nu == 3:
        hs = [0.5 * SX, 0.5 * SY, 0.5 * SZ]
        p["generators"] = np.stack([0 * p["generators"][0]] + [gen(h) for h in hs])
        p["models"] = np.ascontiguousarray(discretize_homogeneous(list(p["generators"]), p["dt"], order)[None])
        p["plant_ops"] = np.stack(hs)[None]
        p["R"] = 1e-2 * np.identity(3)
        p["U_targ"] = np.zeros((3, p["U_targ"].shape[1]))
        p["dim_u"] = 3
    p["gen_op0"] = np.stack([gen(h) for h in p["plant_op0"]])
    p["gen_ops"] = np.stack([gen(h) for h in p["plant_ops"][0]])[None]
    return _tune(p, "process")


# ---------------------------------------------------------------- planned exits
def _planned(xs, state, ns, steps=None):
    """Per member: the planned exit step k_b - steps[b] if given, else b % (ns + 1) with the last member never - and its target,
    the state stored at k_b ('prev') or k_b + 1 ('next'); a member planned at ns has a target no step of this kind ever reads."""
    B, n = xs.shape[0], xs.shape[2]
    if steps is None:
        k = np.array([b % (ns + 1) for b in range(B)])
        k[-1] = ns
    else:
        k = np.asarray(steps)
    target = np.empty((B, n), dtype=complex)
    for b in range(B):
        target[b] = xs[b, min(k[b] + (state == "next"), ns)] if k[b] < ns else xs[b, 0] + 10.0
    return target


def _expected_exit(xs, target, state, ns):
    """First step s whose stored state ('prev': xs[s], 'next': xs[s + 1]) equals the target bit for bit, else None."""
    for s in range(ns):
        x = xs[s] if state == "prev" else xs[s + 1]
        if np.array_equal(x.view(np.float64), target.view(np.float64)):
            return s
    return None


def _check_planned(ref, got, target, state, ns):
    B = ref["xs"].shape[0]
    for b in range(B):
        s = _expected_exit(ref["xs"][b], target[b], state, ns)
        if s is None:
            assert got["exit_codes"][b] == 0 and got["steps_done"][b] == ns, (b, got["exit_codes"][b], got["steps_done"][b])
            for f in ("xs", "us", "qp_solves"):
                assert np.array_equal(got[f][b], ref[f][b]), (b, f)
            continue
        assert got["exit_codes"][b] == 1 and got["steps_done"][b] == s, (b, s, got["exit_codes"][b], got["steps_done"][b])
        assert np.array_equal(got["xs"][b, :s + 2], ref["xs"][b, :s + 2]), b          # (step s ran: its entries are stored)
        assert np.array_equal(got["us"][b, :s + 1], ref["us"][b, :s + 1]), b
        assert np.array_equal(got["qp_solves"][b, :s + 1], ref["qp_solves"][b, :s + 1]), b

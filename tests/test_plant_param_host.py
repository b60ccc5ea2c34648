"""CPU checks of the plant-parameter gradient and of the calibration (mpc4quantum_amd/plant_param.py): the NumPy / SciPy definition
against central differences of its own J and against an independent forward chain, the exact identity with the control gradient,
the fit on noise-free data from perturbed plants, and every ValueError of the Python layer before the library is touched."""
import os

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, plant_param
from tests import grad_cases as gc
from tests import kernel_variants as kv
from tests import plant_param_cases as pc
from tests.test_grad_host import FD_BOUND, H_FD        # the same differencing of the same kind of objective: the same step and bound

B_FD, N_FD = 2, 5
# (plant, p, scale_grad): Hamiltonian d = 2, 3, 4 and the process plant, each at the largest direction count with the drive gains
FD_CASES = [("4-1", 6, True), ("9-2", 2, True), ("16-1", 2, True), ("16-3", 3, False), ("16-1-process", 6, True)]


def _central(J, z):
    g = np.empty(z.shape)
    for j in range(z.shape[1]):
        e = np.zeros(z.shape)
        e[:, j] = H_FD
        g[:, j] = (J(z + e) - J(z - e)) / (2 * H_FD)
    return g


@pytest.mark.parametrize("variant", ["shared", "per"])
@pytest.mark.parametrize("name,p,sg", FD_CASES, ids=lambda v: str(v))
def test_reference_against_central_differences(name, p, sg, variant):
    """shared: a non-uniform grid, col_w with zeros, u_scale; per: per-member operators, sequences, dirs and data."""
    c, args, kw = pc.inputs(name, variant, B_FD, N_FD, p, 9300 + 7 * p + (1 if variant == "per" else 0))
    x0, u, op0, ops, dirs, ts, W, data = args
    ref = m4q.plant_param_grad_reference(*args, scale_grad=sg, **kw)
    assert set(ref) == ({"J", "grad_theta", "grad_scale"} if sg else {"J", "grad_theta"})
    sc = np.ones((B_FD, c.m)) if kw["u_scale"] is None else kw["u_scale"]
    cw = np.ones(N_FD + 1) if kw["col_w"] is None else kw["col_w"]
    # J against the chained independent steps
    o0 = np.broadcast_to(op0.reshape(-1, c.d, c.d), (B_FD, c.d, c.d))
    ok = np.broadcast_to(ops.reshape(-1, c.m, c.d, c.d), (B_FD, c.m, c.d, c.d))
    useq = np.broadcast_to(u.reshape(-1, N_FD, c.m), (B_FD, N_FD, c.m))
    ys = np.broadcast_to(data.reshape(-1, N_FD + 1, c.n), (B_FD, N_FD + 1, c.n))
    dts = np.diff(ts) if np.ndim(ts) else np.full(N_FD, ts)
    xs = np.stack([gc.plant_chain(c, x0[b], sc[b][None, :] * useq[b], o0[b], ok[b], dts) for b in range(B_FD)])
    dd = xs - ys
    J_ind = (cw[None, :] * np.einsum('btj,jk,btk->bt', dd.conj(), W, dd).real).sum(axis=1)
    assert np.abs(ref["J"] - J_ind).max() <= 1e-12 * max(1.0, np.abs(J_ind).max())

    def J_of(theta, s):
        return m4q.plant_param_grad_reference(x0, u, m4q.plant_param_op0(op0, dirs, theta), ops, dirs, ts, W, data, kind=c.kind, u_scale=s,
                                              col_w=kw["col_w"])["J"]
    checks = [("grad_theta", _central(lambda th: J_of(th, sc), np.zeros((B_FD, p))))]
    if sg:
        checks.append(("grad_scale", _central(lambda s: J_of(np.zeros((B_FD, p)), s), sc)))
    for key, fd in checks:
        err = np.abs(ref[key] - fd).max() / max(1.0, np.abs(ref[key]).max())
        print("%s %s %s: max|g| = %.3e, against central differences %.2e" % (name, variant, key, np.abs(ref[key]).max(), err))
        assert ref[key].shape == fd.shape and err <= FD_BOUND
        assert np.abs(ref[key]).max() > 1e-3


def test_unmeasured_columns_are_never_read():
    """A column of weight 0 contributes nothing, whatever data holds there - a NaN included - and the costate passes through it."""
    c, args, kw = pc.inputs("9-2", "shared", 2, 6, 2, 9350)
    ref = m4q.plant_param_grad_reference(*args, scale_grad=True, **kw)
    data = np.array(args[7])
    data[kw["col_w"] == 0.0] = np.nan
    again = m4q.plant_param_grad_reference(*args[:7], data, scale_grad=True, **kw)
    assert all(np.array_equal(ref[k], again[k]) for k in ref) and np.isfinite(ref["grad_theta"]).all()
    assert (kw["col_w"] == 0.0).sum() >= 2 and kw["col_w"][3] == 0.0 and kw["col_w"][6] == 0.0     # (one of them is the last column)


@pytest.mark.parametrize("name", ["4-2", "9-2", "16-1-process"])
def test_direction_of_a_control_operator_is_the_control_gradient(name):
    """dirs = ops and col_w = e_N: J is the control gradient's figure "last" against target = data[:, N], and
    dJ/dtheta_k = sum_t dJ/du[t][k] / u_scale_k - both are sum_t Re(lam_{t+1}^H dx_{t+1}/dv_k) - to rounding."""
    c = gc.plant_case(name)
    B, N = 3, 5
    rng = np.random.default_rng(9400 + c.n + c.m)
    x0 = c.states(rng, B)
    op0, ops = c.member_ops(rng, B)
    u = rng.uniform(-c.sat, c.sat, (N, c.m))
    sc = 1 + 0.1 * rng.standard_normal((B, c.m))
    W, _ = gc.weights_and_targets(rng, c.n, B)
    data = pc.data_for(rng, c, B, N)
    ts = gc.grid(rng, N, c.dt)
    cw = np.zeros(N + 1)
    cw[N] = 1.0
    par = m4q.plant_param_grad_reference(x0, u, op0, ops, ops, ts, W, data, c.kind, u_scale=sc, col_w=cw, scale_grad=(2 * c.m <= pc.p_max(name)))
    ctl = m4q.plant_rollout_grad_reference(x0, u, op0, ops, ts, W, data[:, N], c.kind, u_scale=sc, figure="last")
    want = ctl["grad"].sum(axis=1) / sc
    scale = max(1.0, np.abs(want).max())
    assert np.abs(par["J"] - ctl["q"]).max() <= 1e-13 * max(1.0, np.abs(ctl["q"]).max())
    assert np.abs(par["grad_theta"] - want).max() <= 1e-12 * scale and np.abs(want).max() > 1e-3
    if "grad_scale" in par:
        assert np.abs(par["grad_scale"] - ctl["grad_scale"]).max() <= 1e-12 * max(1.0, np.abs(ctl["grad_scale"]).max())


# ---------------------------------------------------------------- the direction-count matrix
def test_param_rule_lines_read_as_mirrored():
    """kernel_variants.param_cells() / param_waves() against the lines of m4q_kernels.hip they were written from."""
    with open(os.path.join(kv.CSRC, "m4q_kernels.hip")) as fh:
        k = fh.read()
    for line in ("  if constexpr ((1 + PT) * D > 16) {\n    return UNBUILT;\n",
                 "    return launch_param_pt<PLANT, PT + 1>(a, p_tot, s);\n",
                 "    const auto go = [&](auto plant) { return launch_param_pt<decltype(plant)::value, 1>(a, p_tot, s); };\n",
                 "constexpr int param_waves() { return (1 + PT) * (PLANT == PLANT_PROCESS ? DQ : DD) > 6 ? 1 : WAVES; }\n",
                 "constexpr int WAVES = NX <= 9 ? 2 : 1;\n"):
        assert k.count(line) == 1, line
    assert k.count("#if !defined(M4Q_NO_AUX) && M4Q_ORDER == 1\n") == 2                  # the kernel; its launcher
    assert k.count("  constexpr int D = PLANT == PLANT_PROCESS ? DQ : DD;\n") >= 2
    body = k[k.index("static int launch_param_by_plant("):k.index("static int launch_plant_param_grad(")]
    assert body.count("  if constexpr (!SQUARE) {\n    return UNBUILT;\n") == 1
    assert body.count("    if (a.roll.kind == PLANT_HAMILTONIAN) return go(ic<PLANT_HAMILTONIAN>{});\n") == 1
    assert body.count("      if constexpr (QUARTIC) return go(ic<PLANT_PROCESS>{});\n      else return UNBUILT;\n") == 1


def test_param_cells_are_the_built_instances():
    H, P = kv.HAMILTONIAN, kv.PROCESS
    want = [(4, 1, H, 7), (4, 2, H, 7), (9, 2, H, 4), (16, 1, H, 3), (16, 3, H, 3), (16, 1, P, 7), (16, 3, P, 7)]
    cells = kv.param_cells()
    assert cells == [(nx, nu, kind, pt) for nx, nu, kind, top in want for pt in range(1, top + 1)]
    assert len(cells) == 38 == len(set(cells)) and 14 + 4 + 6 + 14 == 38
    for nx, nu, kind, top in want:
        d = kv.param_dim(nx, kind)
        assert plant_param.max_directions(d) == top and (1 + top) * d <= 16 < (2 + top) * d
        assert gc.plant_case(pc.cell_name(nx, nu, kind)).d == d and pc.p_max(pc.cell_name(nx, nu, kind)) == top
    # the occupancy switch: one wave per SIMD past 6 columns - from PT = 3 at d = 2, from PT = 2 at d = 3, always at d = 4
    assert [kv.param_waves(4, H, pt) for pt in range(1, 8)] == [2, 2, 1, 1, 1, 1, 1]
    assert [kv.param_waves(9, H, pt) for pt in range(1, 5)] == [2, 1, 1, 1]
    assert {kv.param_waves(16, kind, pt) for kind in (H, P) for pt in range(1, 4)} == {1}
    # the matrix runs every cell at both splits, in both layouts
    cases = pc.matrix_cases()
    assert {(name, pt) for name, pt, p, sg, v in cases} == {(pc.cell_name(nx, nu, kind), pt) for nx, nu, kind, pt in cells}
    assert len(cases) == 2 * (13 + 12 + 6 + 5 + 3 + 13 + 11) == len({pc.matrix_id(c) for c in cases})
    for name, pt, p, sg, v in cases:
        m = gc.plant_case(name).m
        assert p >= 1 and p + (m if sg else 0) == pt
    assert not [1 for name, pt, p, sg, v in cases if name == "16-3" and sg]                # (d = 4, m = 3: no room for the gains)


MATRIX = pc.matrix_cases()


@pytest.mark.parametrize("case", MATRIX, ids=[pc.matrix_id(c) for c in MATRIX])
def test_matrix_cases_tell_their_directions_apart(case):
    """On the definition alone: every column of [grad_theta, grad_scale] is non-trivial (max_b |g[:, j]| > 1e-3) and no two columns
    lie within 1e-6 max|ref| of each other - a swapped or repeated direction, or a gain stored into a theta slot, is far outside
    the device's bound of 1e-10 max(1, max|ref|)."""
    c, args, kw = pc.matrix_inputs(case)
    name, pt, p, sg, variant = case
    ref = m4q.plant_param_grad_reference(*args, scale_grad=sg, **kw)
    assert ref["grad_theta"].shape == (pc.MATRIX_B, p) and (not sg or ref["grad_scale"].shape == (pc.MATRIX_B, c.m))
    small, near = pc.columns(ref)
    print("%s: smallest column maximum %.3e, nearest two columns %.3e max|ref|" % (pc.matrix_id(case), small, near))
    assert small > 1e-3 and near > 1e-6
    assert all(args[4][..., j, :, :].any() for j in range(p))
    assert set(pc.MATRIX_RESEED) <= {pc.matrix_id(c) for c in MATRIX}


# ---------------------------------------------------------------- the fit
@pytest.fixture(scope="module")
def fitted():
    cal = pc.calibration_case()
    trace = []
    out = m4q.plant_calibrate_reference(*cal.args(cal.data_reference()), trace=trace, **cal.kwargs())
    return cal, out, trace


def test_calibration_recovers_the_parameters(fitted):
    """Every member of the case set converges (status 1, none admitted otherwise).  At a stop every entry of the gradient is at
    most gtol = 1e-7 (no bound is active at the truth); the Hessian of J in theta at the truth - central differences of the
    definition's gradient - has its smallest eigenvalue between 1.2 and 2.7 over the six members, so the parameters lie within
    sqrt(2) 1e-7 / 1.2 = 1.2e-7 of the truth to first order.  The bound is 1e-6: that, with room for the Hessian's change nearby."""
    cal, out, _ = fitted
    print("status", out["status"], "n_iter", out["n_iter"], "max error", np.abs(out["theta"] - cal.theta_true).max(axis=1))
    assert np.array_equal(out["status"], np.full(cal.B, plant_param.STATUS_CONVERGED))
    assert np.abs(out["theta"] - cal.theta_true).max() <= 1e-6
    assert np.abs(out["theta"][1:] - cal.theta0[1:]).max() > 1e-2                  # (they had somewhere to go)
    assert np.array_equal(out["op0"], m4q.plant_param_op0(cal.c.op0, cal.dirs, out["theta"]))
    assert np.all(out["cost"][1:] < 1e-10) and np.all(out["cost_hist"][1:, 0] > 1e-4)


def test_calibration_cost_history_is_monotone(fitted):
    cal, out, trace = fitted
    assert out["cost_hist"].shape == (cal.B, cal.ITERS + 1) and np.all(np.diff(out["cost_hist"], axis=1) <= 0)
    assert np.array_equal(out["cost_hist"][:, -1], out["cost"])
    for b in range(cal.B):
        k = out["n_iter"][b]
        assert np.all(out["alpha_hist"][b, k:] == 0) and np.all(out["cost_hist"][b, k:] == out["cost"][b])
    assert len(trace) == out["n_iter"].max()


def test_member_at_the_truth_stops_at_once(fitted):
    cal, out, _ = fitted
    assert out["n_iter"][0] == 0 and out["status"][0] == plant_param.STATUS_CONVERGED and out["cost"][0] == 0.0
    assert np.array_equal(out["theta"][0], cal.theta_true[0]) and np.all(out["n_iter"][1:] >= 3)


def test_calibration_respects_bounds_and_members_do_not_see_each_other(fitted):
    cal, out, _ = fitted
    lo, hi = cal.bounds
    assert np.all(out["theta"] >= lo) and np.all(out["theta"] <= hi)
    # a box that cuts the truth off: the fit ends on the box, inside it
    tight = (-0.05 * cal.scale, 0.05 * cal.scale)
    kw = dict(cal.kwargs(), bounds=tight, theta0=np.zeros((cal.B, cal.p)))
    cut = m4q.plant_calibrate_reference(*cal.args(cal.data_reference()), **kw)
    assert np.all(cut["theta"] >= tight[0]) and np.all(cut["theta"] <= tight[1])
    outside = np.abs(cal.theta_true) > 0.05 * cal.scale
    assert outside.any() and np.all(np.abs(cut["theta"][outside]) == np.broadcast_to(0.05 * cal.scale, outside.shape)[outside])
    assert np.all(np.diff(cut["cost_hist"], axis=1) <= 0)
    # members 2 .. 4 alone: the same run, bit for bit
    idx = slice(2, 5)
    x0, u, op0, ops, dirs, dt, W, data = cal.args(cal.data_reference())
    kw = dict(cal.kwargs(), theta0=cal.theta0[idx])
    part = m4q.plant_calibrate_reference(x0[idx], u, op0, ops, dirs, dt, W, data[idx], **kw)
    for key in ("theta", "cost", "cost_hist", "alpha_hist", "n_iter", "status"):
        assert np.array_equal(part[key], out[key][idx]), key


def test_calibration_fits_the_drive_gains_too():
    """fit_scale on the d = 2 plant (p = 1 detuning and the gain of its one drive): both recovered from noise-free data."""
    c = gc.plant_case("4-1")
    B, N = 3, 10
    rng = np.random.default_rng(9500)
    dirs = pc.physical_directions(2)[:1]
    theta = rng.uniform(-0.05, 0.05, (B, 1))
    sc = 1 + rng.uniform(-0.1, 0.1, (B, 1))
    x0 = c.states(rng, B)
    u = rng.uniform(-c.sat, c.sat, (N, 1))
    o0 = m4q.plant_param_op0(c.op0, dirs, theta)
    dts = np.full(N, c.dt)
    data = np.stack([plant_param.member_states(x0[b], sc[b][None, :] * u, o0[b], c.ops, dts, c.kind) for b in range(B)])
    out = m4q.plant_calibrate_reference(x0, u, c.op0, c.ops, dirs, c.dt, np.eye(4), data, fit_scale=True, iters=60, steps=8, tol=0.0,
                                        gtol=1e-8, step0=0.05)
    print("status", out["status"], "n_iter", out["n_iter"], "cost", out["cost"])
    assert np.array_equal(out["status"], np.ones(B)) and set(out) >= {"theta", "u_scale", "op0"}
    assert np.abs(out["theta"] - theta).max() <= 1e-5 and np.abs(out["u_scale"] - sc).max() <= 1e-5


def test_loop_runs_on_any_evaluator():
    """evaluate=: a quadratic bowl per member, one of them against its box; a NaN start is status 3; no descent is status 2."""
    A = np.array([[[3.0, 0.5], [0.5, 1.0]], [[1.0, 0.0], [0.0, 40.0]], [[2.0, 0.0], [0.0, 2.0]]])
    zs = np.array([[1.0, -2.0], [0.5, 0.25], [5.0, 0.0]])

    def bowl(z):
        dz = z - zs
        g = np.einsum('bij,bj->bi', A, dz)
        return 0.5 * np.sum(dz * g, axis=1), g
    cal = pc.calibration_case()
    lo, hi = np.full((3, 2), -np.inf), np.full((3, 2), np.inf)
    hi[2, 0] = 3.0
    out = plant_param.calibrate_loop(np.zeros((3, 2)), lo, hi, bowl, iters=60, mem=5, steps=10, step0=0.5, tol=0.0, gtol=1e-10)
    assert np.array_equal(out["status"], [1, 1, 1])
    assert np.abs(out["z"][:2] - zs[:2]).max() <= 1e-8 and out["z"][2, 0] == 3.0 and abs(out["z"][2, 1]) <= 1e-8
    nan = plant_param.calibrate_loop(np.zeros((2, 2)), lo[:2], hi[:2], lambda z: (np.array([np.nan, 1.0]) + 0 * z[:, 0], np.ones((2, 2))),
                                     iters=3, steps=2)
    assert nan["status"][0] == plant_param.STATUS_NOT_FINITE and nan["n_iter"][0] == 0
    assert nan["status"][1] == plant_param.STATUS_NO_DESCENT and nan["n_iter"][1] == 1      # (a constant J with a gradient: nothing descends)
    assert cal.B == 6


# ---------------------------------------------------------------- refusals of the Python layer
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _args(B=3, n=9, m=2, N=4, d=3, p=2):
    return dict(x0=np.zeros((B, n), complex), us=np.zeros((N, m)), op0=np.zeros((d, d), complex), ops=np.zeros((m, d, d), complex),
                dirs=pc.physical_directions(d)[:p], dt_or_ts=0.25, W=np.eye(n), data=np.zeros((B, N + 1, n), complex))


NOT_HERMITIAN = np.array([[[0, 1, 0], [0, 0, 0], [0, 0, 0]]], dtype=complex)
BAD = [dict(dirs=NOT_HERMITIAN), dict(dirs=np.eye(3) * 1j), dict(dirs=np.zeros((2, 2, 2))), dict(dirs=np.zeros((0, 3, 3))),
       dict(dirs=np.zeros((2, 2, 3, 3))), dict(dirs=np.zeros((3, 3))), dict(dirs=None), dict(dirs=np.full((1, 3, 3), np.nan)),
       dict(data=np.zeros((3, 4, 9))), dict(data=np.zeros((3, 5, 4))), dict(data=np.zeros((2, 5, 9))), dict(data=np.zeros(9)), dict(data=None),
       dict(col_w=np.ones(4)), dict(col_w=np.ones((5, 1))), dict(col_w=[1, 1, -1, 1, 1]), dict(col_w=[1, np.nan, 1, 1, 1]),
       dict(col_w=[1, np.inf, 1, 1, 1]), dict(W=None), dict(W=np.eye(4)), dict(x0=np.zeros(9)), dict(us=np.zeros(4)),
       dict(u_scale=np.ones((3, 1))), dict(op0=np.zeros((2, 2))), dict(dt_or_ts=np.zeros(3)),
       dict(kind=_lib.PLANT_GENERATOR), dict(kind=_lib.PLANT_NONE), dict(kind=_lib.PLANT_PROCESS)]


@pytest.mark.parametrize("change", BAD, ids=lambda c: ",".join("%s%s" % (k, getattr(v, "shape", v)) for k, v in c.items()))
def test_wrappers_refuse_bad_arguments(no_library, change):
    for fn in (m4q.plant_rollout_param_grad_batch, m4q.plant_param_grad_reference, m4q.plant_calibrate_batch, m4q.plant_calibrate_reference):
        with pytest.raises(ValueError):
            fn(**dict(_args(), **change))


@pytest.mark.parametrize("n,d,m,p,sg,limit", [(4, 2, 1, 8, False, 7), (4, 2, 1, 7, True, 7), (9, 3, 2, 5, False, 4), (9, 3, 2, 3, True, 4),
                                               (16, 4, 3, 4, False, 3), (16, 4, 3, 1, True, 3)])
def test_too_many_directions_name_the_limit(no_library, n, d, m, p, sg, limit):
    a = _args(n=n, m=m, d=d)
    a["dirs"] = np.stack([np.eye(d, dtype=complex)] * p)
    with pytest.raises(ValueError, match="at most %d directions" % limit):
        m4q.plant_rollout_param_grad_batch(scale_grad=sg, **a)
    with pytest.raises(ValueError, match="at most %d directions" % limit):
        m4q.plant_calibrate_batch(fit_scale=sg, **a)
    assert plant_param.max_directions(d) == limit


def test_generator_plant_and_bad_fit_parameters_are_refused(no_library):
    with pytest.raises(ValueError, match="generator"):
        m4q.plant_rollout_param_grad_batch(**dict(_args(), op0=np.zeros((9, 9)), ops=np.zeros((2, 9, 9)), dirs=np.zeros((1, 9, 9)),
                                                  kind=_lib.PLANT_GENERATOR))
    for bad in (dict(iters=0), dict(steps=0), dict(mem=-1), dict(step0=0.0), dict(tol=-1.0), dict(gtol=np.nan), dict(theta0=np.zeros((3, 3))),
                dict(theta0=np.full((3, 2), np.nan)), dict(bounds=(1.0, -1.0)), dict(bounds=(np.zeros(3), np.ones(3))), dict(bounds=(np.nan, 1.0))):
        with pytest.raises((ValueError, TypeError)):
            m4q.plant_calibrate_batch(**dict(_args(), **bad))
    x0, ts = np.zeros((3, 9), complex), np.arange(5) * 0.25
    with pytest.raises(ValueError, match="generator"):
        m4q.LExperiment(np.eye(9), [np.eye(9)] * 2).calibrate_batch(x0, ts, np.zeros((2, 5)), np.zeros((1, 9, 9)), np.eye(9), np.zeros((3, 5, 9)))
    exp = m4q.QExperiment(np.diag([0.0, 1.0, 2.0]), [np.eye(3), np.eye(3)])
    with pytest.raises(ValueError):
        exp.calibrate_batch(x0, ts, np.zeros((2, 5)), NOT_HERMITIAN, np.eye(9), np.zeros((3, 5, 9)))
    exp.set("c_ops", [0.2 * np.diag(np.sqrt(np.arange(1, 3)), 1).astype(complex)])
    with pytest.raises(ValueError, match="generator"):
        exp.calibrate_batch(x0, ts, np.zeros((2, 5)), pc.physical_directions(3), np.eye(9), np.zeros((3, 5, 9)))


def test_wrapper_hands_the_kernel_what_it_was_given(monkeypatch):
    seen = {}

    class Fake:
        def m4q_plant_rollout_param_grad_batch(self, *a):
            seen["a"] = a
            return 0

        def m4q_last_error(self):
            return b""
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    B, n, m, N, p = 3, 9, 2, 4, 2
    ts = np.array([0.0, 0.1, 0.35, 0.4, 1.0])
    a = _args()
    dirs = np.stack([pc.physical_directions(3)] * B)
    out = m4q.plant_rollout_param_grad_batch(a["x0"], a["us"], a["op0"], a["ops"], dirs, ts, a["W"], a["data"][0], u_scale=np.ones((B, m)),
                                             col_w=[1.0, 0.0, 2.0, 0.0, 1.0], scale_grad=True)
    s = seen["a"]
    assert len(s) == 23 and s[:5] == (B, n, m, _lib.PLANT_HAMILTONIAN, N) and s[8] == 0 and s[9] is not None and s[12] == 0
    assert s[13] == p and s[15] == 1 and s[18] == 0 and s[22] is not None
    assert np.array_equal(np.ctypeslib.as_array(s[5], (N,)), np.diff(ts))
    assert np.array_equal(np.ctypeslib.as_array(s[19], (N + 1,)), [1.0, 0.0, 2.0, 0.0, 1.0])
    assert set(out) == {"J", "grad_theta", "grad_scale"} and out["grad_theta"].shape == (B, p) and out["grad_scale"].shape == (B, m)
    out = m4q.plant_rollout_param_grad_batch(a["x0"], np.zeros((B, N, m)), np.zeros((B, 3, 3)), a["ops"], dirs[0], 0.5, a["W"], a["data"])
    s = seen["a"]
    assert s[8] == 1 and s[9] is None and s[12] == 1 and s[15] == 0 and s[18] == 1 and s[22] is None
    assert np.array_equal(np.ctypeslib.as_array(s[19], (N + 1,)), np.ones(N + 1)) and set(out) == {"J", "grad_theta"}


def test_prototypes_and_exports():
    assert len(_lib.PROTOTYPES["m4q_plant_rollout_param_grad_batch"][1]) == 23
    assert m4q.plant_rollout_param_grad_batch is plant_param.plant_rollout_param_grad_batch
    assert m4q.plant_calibrate_batch is plant_param.plant_calibrate_batch
    for cls in (m4q.QExperiment, m4q.LExperiment, m4q.QSynthesis):
        assert callable(cls.calibrate_batch)


# ---------------------------------------------------------------- refusals of the C ABI, before a device is asked for
class _Call:
    """m4q_plant_rollout_param_grad_batch on all-zero data of consistent sizes; call(**changes) returns the code."""

    def __init__(self, B=2, n=9, m=2, N=3, d=3, p=2, kind=_lib.PLANT_HAMILTONIAN):
        z = lambda *s: np.zeros(s)                                                   # noqa: E731
        self.v = dict(B=B, n=n, m=m, kind=kind, N=N, dts=np.full(N, 0.25), x0=z(B, n, 2), u=z(N, m), u_per=0, u_scale=None,
                      op0=z(d, d, 2), ops=z(m, d, d, 2), per=0, p=p, dirs=z(p, d, d, 2), d_per=0, W=z(n, n, 2), data=z(N + 1, n, 2),
                      y_per=0, col_w=None, J=z(B), gt=z(B, p), gs=None)

    def __call__(self, **changes):
        v = dict(self.v, **changes)
        k = {key: (np.ascontiguousarray(x, dtype=np.float64) if isinstance(x, (np.ndarray, list)) else x) for key, x in v.items()}
        ptr = lambda a: None if a is None else a.ctypes.data_as(_lib._dp)                                             # noqa: E731
        return _lib.lib().m4q_plant_rollout_param_grad_batch(k["B"], k["n"], k["m"], k["kind"], k["N"], ptr(k["dts"]), ptr(k["x0"]),
                                                             ptr(k["u"]), k["u_per"], ptr(k["u_scale"]), ptr(k["op0"]), ptr(k["ops"]),
                                                             k["per"], k["p"], ptr(k["dirs"]), k["d_per"], ptr(k["W"]), ptr(k["data"]),
                                                             k["y_per"], ptr(k["col_w"]), ptr(k["J"]), ptr(k["gt"]), ptr(k["gs"]))


def _err():
    return _lib.lib().m4q_last_error()


@pytest.mark.parametrize("change", [dict(B=0), dict(N=0), dict(p=0), dict(x0=None), dict(u=None), dict(W=None), dict(data=None), dict(dts=None),
                                    dict(op0=None), dict(ops=None), dict(dirs=None), dict(J=None), dict(gt=None), dict(kind=_lib.PLANT_NONE),
                                    dict(kind=4), dict(kind=_lib.PLANT_PROCESS), dict(col_w=[1.0, -1.0, 1.0, 1.0]),
                                    dict(col_w=[1.0, np.nan, 1.0, 1.0])], ids=str)
def test_c_entry_refuses_bad_arguments(change):
    """(kind = PROCESS on n = 9: not a fourth power.)"""
    assert _Call()(**change) == _lib.E_BADARG
    assert b"m4q_plant_rollout_param_grad_batch" in _err()


def test_c_entry_refuses_what_has_no_kernel():
    who = b"m4q_plant_rollout_param_grad_batch"
    assert _Call(n=25, d=5)() == _lib.E_UNSUPPORTED and who in _err()                    # no compiled shape
    assert _Call(n=8, m=2, d=2)() == _lib.E_UNSUPPORTED and who in _err()                # a shape with a model and no device plant
    assert _Call(n=16, m=2, d=4)() == _lib.E_UNSUPPORTED                                 # the plant-only shape
    assert who in _err() and b"plant-only" in _err()
    assert _Call(n=9, d=9, p=1, kind=_lib.PLANT_GENERATOR)() == _lib.E_UNSUPPORTED       # the generator plant
    assert who in _err() and b"generator" in _err()
    assert _Call(p=5)() == _lib.E_UNSUPPORTED                                            # d = 3: at most 4 directions
    assert who in _err() and b"at most 4 directions for d = 3" in _err()
    c = _Call(p=3)
    assert c(gs=np.zeros((2, 2))) == _lib.E_UNSUPPORTED and b"at most 4 directions for d = 3" in _err()     # 3 + m = 5
    assert _Call(n=4, m=1, d=2, p=8)() == _lib.E_UNSUPPORTED and b"at most 7 directions for d = 2" in _err()
    assert _Call(n=16, m=3, d=4, p=4)() == _lib.E_UNSUPPORTED and b"at most 3 directions for d = 4" in _err()
    assert _Call(n=16, m=1, d=2, p=8, kind=_lib.PLANT_PROCESS)() == _lib.E_UNSUPPORTED and b"at most 7 directions for d = 2" in _err()


def test_well_formed_calls_reach_the_device():
    """Every check passed: the call asks for a device (and, where there is one, runs on the all-zero data)."""
    want = 0 if _lib.device_count() > 0 else _lib.E_NODEVICE
    assert _Call()() == want
    assert _Call(p=4)() == want
    assert _Call(p=2)(gs=np.zeros((2, 2))) == want
    assert _Call(n=4, m=1, d=2, p=7)() == want
    assert _Call(n=16, m=3, d=4, p=3)() == want
    assert _Call(n=16, m=1, d=2, p=6, kind=_lib.PLANT_PROCESS)(gs=np.zeros((2, 1))) == want

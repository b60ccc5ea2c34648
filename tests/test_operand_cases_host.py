"""CPU preconditions of tests/operand_cases.py: what must hold of every (shape, plant, solve, family) before
tests/test_gpu_operand_matrix.py may hold the device to fixed bounds on it.

Each is a condition, not a measurement: a scenario that misses one gets its knobs changed (operand_cases.EPS, THETA, the per-member
spreads, kv.TUNING), never the cap.  The caps are a tenth of the GPU file's bounds (conditioning) and 1e4 times them
(discrimination: a kernel that reads another member's operand, or holds a moving target still, cannot pass).

Rule-based exceptions, by name: the trace condition is that of the traceless paths and is asked of the density-matrix shapes (the
process vectors of the process cells run the complex path alone and have no common trace); the process cells have one nominal
model, so the moving family's model swap does not exist for them."""
import numpy as np
import pytest

from tests import kernel_variants as kv
from tests import operand_cases as oc

KEYS = oc.oracle_keys()


def test_every_cell_has_both_families():
    cells = kv.closed_loop_cells()
    for c in cells:
        for family in oc.FAMILIES:
            p = oc.scenario_of(c, family)
            assert (p["batch"], p["horizon"], p["n_steps"]) == (kv.BATCH, kv.HORIZON, kv.STEPS)
            assert oc.expected_path(c, family) == (kv.TRACELESS if (c.path == kv.TILE and family == oc.MOVING) else c.path)
    only = [c for c in cells if oc.only_through_moving(c)]
    # the general sweep and rollout at n = 8 on the traceless coordinates (the one-index-per-trip rollout beside the pair form) and
    # every exact cell of the real paths are among them; no complex cell is
    assert any((c.nx, c.path, c.exact) == (9, kv.TRACELESS, False) for c in only)
    assert all(c in only for c in cells if c.exact and c.path in (kv.REAL, kv.TRACELESS, kv.TILE))
    assert not any(c.path == kv.COMPLEX for c in only)


def _columns(X):
    """[B | 1, cols, n]: the target columns, member by member."""
    X = np.asarray(X)
    return np.swapaxes(X if X.ndim == 3 else X[None], 1, 2)


@pytest.mark.parametrize("key", KEYS, ids=oc.key_id)
def test_scenario_preconditions(key):
    nx, nu, order, plant, exact, family, sg = key
    p, xs, us, codes, solves, trace = oc._oracle(*key)
    B, ns, sat, m = p["batch"], p["n_steps"], p["sat"], p["dim_u"]
    process = plant == kv.PROCESS
    assert np.all(codes == 0), codes
    assert np.abs(us).max() <= sat * (1 + 1e-15)

    # ---- layout: what the family says of strides and columns
    cols = _columns(p["X_targ"])
    if family == oc.PER:
        assert p["target_per"] and p["plant_per"] and cols.shape[0] == B and p["U_targ"].shape[0] == B
        for b in range(B):
            assert all(cols[b, c].tobytes() == cols[b, 0].tobytes() for c in range(cols.shape[1])), b    # bit-identical columns
        assert len({cols[b, 0].tobytes() for b in range(B)}) == B
        assert len({p["U_targ"][b, :, 0].tobytes() for b in range(B)}) == B                            # u_prev of steps 0, 1 differs
        assert p["model_per"] == (not process) and p["models"].shape[0] == (1 if process else B)
    else:
        assert not p["target_per"] and not p["plant_per"] and cols.shape[0] == 1 and p["model_per"] == sg
        assert p["models"].shape[0] == (B if sg else 1)
        assert min(np.abs(cols[0, c] - cols[0, 0]).max() for c in range(1, cols.shape[1])) > 1e-3
        assert len({x.tobytes() for x in p["x0"]}) == B
    # ---- one trace for states and targets (a tenth of the session's own threshold; density-matrix shapes)
    for sl, d in oc._blocks(nx, process):
        tr = np.concatenate([[np.trace(x[sl].reshape(d, d)) for x in p["x0"]],
                             [np.trace(x[sl].reshape(d, d)) for x in cols.reshape(-1, cols.shape[2])]])
        assert np.abs(tr.imag).max() <= 1e-13
        assert tr.real.max() - tr.real.min() <= 1e-13 * max(1.0, np.abs(tr.real).max())

    # ---- the box is exercised, and the exact solve is not the clipped one
    near = sat * (1 - 1e-9)
    at_bound = int((np.abs(us) >= near).sum()) + sum(int((np.abs(trace[b][k][1]) >= near).sum()) for b in range(B) for k in range(ns + 1))
    assert at_bound > 0, "no control or guess entry at the bound"
    if exact:
        clip = oc._oracle(nx, nu, order, plant, False, family, sg)[2]
        assert np.abs(us - clip).max() > 1e-3 * sat
    if family == oc.PER:
        assert len({tuple(s) for s in solves}) > 1, solves

    # ---- conditioning: a tenth of the GPU bounds on every step and member
    for b in range(B):
        for k in range(ns):
            su, sx, sxg, sug = oc.step_sensitivity(p, plant, exact, b, k, xs, us, trace[b][k])
            if exact:
                assert su / sat <= 1e-10 and sx <= 1e-10, (b, k, su / sat, sx)
            else:
                assert su <= 1e-11 and sx <= 1e-11 and sxg <= 1e-8 and sug <= 1e-8, (b, k, su, sx, sxg, sug)

    # ---- discrimination: 1e-6 sat on the applied controls of some step
    def moved(b, **over):
        q = oc.member(p, b)
        got = oc.run_oracle(q, plant, exact, **over)[1][0]
        return np.abs(got - us[b]).max() / sat

    if family == oc.PER:
        op0_key, ops_key = ("plant_op0", "plant_ops") if plant == kv.HAMILTONIAN else ("gen_op0", "gen_ops")
        for b in range(B):
            nb = (b + 1) % B
            for name, over in (("X_targ", dict(X_targ=p["X_targ"][nb])), ("U_targ", dict(U_targ=p["U_targ"][nb])),
                               ("op0", {op0_key: p[op0_key][nb:nb + 1]}), ("ops", {ops_key: p[ops_key][nb:nb + 1]})):
                assert moved(b, **over) >= 1e-6, (b, name)
    else:
        held = np.tile(p["X_targ"][:, :1], (1, p["X_targ"].shape[1]))
        base = oc._base(nx, nu, order, process)
        for b in range(B):
            assert moved(b, X_targ=held) >= 1e-6, (b, "target held at column 0")
            if not process:
                other = p["models"][(b + 1) % B] if sg else base["models"][1]
                assert moved(b, models=other[None]) >= 1e-6, (b, "model")

"""Launch schedules against single steps, every kernel variant with a device plant (-m gpu).

One launch cuts each member's run into work items (kernel_variants.pieces: a head [begin, 2), the rest, and in exact mode the rest
again at XCUTS), hands the SQP guess from item to item through device memory (on the real paths as a flat copy in the kernel's own
coordinates) and lets each resident row run member after member in the same workspace.  tests/test_gpu_variant_matrix.py runs
every step as its own launch of five members, which exercises none of that.  Here every closed-loop cell with a device plant
(PLANT_NONE cells take every state from the host) runs its scenario for LONG_STEPS steps, and the one launch run(0, 14) of the
five members is the reference:

(a) its head piece (steps 0 and 1 with all their SQP iterations) against the oracle's run of the same scenario, and its QP-solve
    counts on all 14 steps;
(b) the chain of single-step launches and the two-launch resumes at every cut and one step either side: identical bits on the
    complex path; on the real paths identical counts and codes, us / xs within 1e-10 and the final guesses within 1e-7 (the
    matrix's per-step tolerances: a launch boundary hands the guess over through the complex basis, a cut inside a launch does
    not);
(c) a checkpoint restored into a fresh session resumes bit for bit as the same session does;
(d) the five members among thousands of others on a capped grid - every row runs four members or more, tails land on other rows
    than their heads, fillers exit at planned steps in every piece or fail at step 0 - and each alone (B = 1): bit for bit;
(e) exact cells: planned exits at steps spread over all five pieces of the launch."""
import functools

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from mpc4quantum_amd.configs import rx
from oracle import m4q_oracle as orc
from tests import kernel_variants as kv
from tests.kernel_variants import _check_planned, _planned
from tests.test_gpu_variant_matrix import _open, _plant_ops

pytestmark = pytest.mark.gpu

NS = kv.LONG_STEPS
PLANT_CELLS = [c for c in kv.closed_loop_cells() if c.plant != kv.NONE]
OUTPUTS = ("xs", "us", "qp_solves", "exit_codes", "steps_done")
RESUME_AT = (1, 2, 3, 4, 5, 7, 8, 12, 13)          # every cut (2 and XCUTS) and one step either side
CHECKPOINT_AT = (2, 7)
EXIT_STEPS = (0, 1, 2, 3, 4, 6, 7, 11, 12, 13)     # (e): two or more in each of the five exact pieces
# (d): 16 members per workgroup of a grid capped at one workgroup per CU (256 on an MI355X) and three more - the final wavefront
# holds three members and one idle row
BIG = 16 * 256 + 3
LATE = 256                                         # "drawn late": among the last heads the queue hands out
PER_MEMBER = ("x0", "models", "scales", "plant_op0", "gen_op0")


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


def _same(a, b):
    """Identical bits (floating-point fields compared as integers: -0.0 is not 0.0, a NaN equals its own bits)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint64), b.view(np.uint64)) if a.dtype.kind in "fc" else np.array_equal(a, b)


@functools.lru_cache(maxsize=8)
def _scenario_of(nx, nu, order, process, batch):
    if process:
        return kv.process_scenario(nu, order, batch=batch, n_steps=NS)
    return kv.scenario(nx, nu, order, batch=batch, n_steps=NS)


def _scenario(cell, batch=kv.BATCH):
    """The cell's scenario at LONG_STEPS (cached: callers do not modify it)."""
    return _scenario_of(cell.nx, cell.nu, cell.order, cell.plant == kv.PROCESS, batch)


def _take(p, idx):
    """Scenario p restricted to (or repeated over) the members idx: every per-member input indexed, shared ones kept."""
    q = dict(p, batch=len(idx))
    for key in PER_MEMBER:
        v = p.get(key)
        if v is not None and p["batch"] > 1 and len(v) == p["batch"]:
            q[key] = np.array(v[np.asarray(idx)])
    return q


def _snapshot(sess):
    """The outputs of the launches so far and the SQP guess the last one left behind."""
    r = sess.results()
    st = sess.state()
    out = {f: r[f] for f in OUTPUTS}
    out["x_guess"], out["u_guess"] = st["x_guess"], st["u_guess"]
    return out


def _reference(cell, p):
    """run(0, 14) of scenario p in one launch."""
    sess = _open(cell, p)
    try:
        assert sess.path_detail() == cell.path
        sess.run(0, NS)
        ref = _snapshot(sess)
        assert sess.path_detail() == cell.path
    finally:
        sess.close()
    assert np.all(ref["exit_codes"] == 0) and np.all(ref["steps_done"] == NS), (ref["exit_codes"], ref["steps_done"])
    return ref


# ---------------------------------------------------------------- (a) the head piece against the oracle
_ORACLE = {}


def _oracle(cell):
    """The oracle's 14-step run of the cell's scenario, time-major (cached per shape, plant and solve: every path shares it)."""
    key = (cell.nx, cell.nu, cell.order, cell.plant, cell.exact)
    if key not in _ORACLE:
        p = _scenario(cell)
        op0, ops, gen = _plant_ops(p, cell.plant)
        xs, us, codes, solves = orc.mpc_batch(p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], p["dt"],
                                              p["horizon"], NS, op0, list(ops[0]), p["Q"], p["R"], p["Qf"], p["sat"], p["du"],
                                              qp_mode="exact" if cell.exact else "qp", generator_plant=gen)
        _ORACLE[key] = (np.swapaxes(xs, 1, 2), np.swapaxes(us, 1, 2), codes, solves)
    return _ORACLE[key]


@pytest.mark.parametrize("cell", PLANT_CELLS, ids=kv.cell_id)
def test_head_piece_matches_the_oracle(cell, record_property):
    """Steps 0 and 1 of the one launch - its head piece, every SQP iteration - against the oracle's free run of the same scenario:
    us[:, 0:2] and xs[:, 1:3] to 1e-10; QP-solve counts identical on all 14 steps; exit codes 0."""
    xs_t, us_t, codes, solves = _oracle(cell)
    assert np.all(codes == 0)
    ref = _reference(cell, _scenario(cell))
    assert np.array_equal(ref["qp_solves"], solves), (ref["qp_solves"], solves)
    eu, ex = rel(ref["us"][:, 0:2], us_t[:, 0:2]), rel(ref["xs"][:, 1:3], xs_t[:, 1:3])
    record_property("head_vs_oracle", [eu, ex])
    assert eu <= 1e-10 and ex <= 1e-10, (eu, ex)


# ---------------------------------------------------------------- (b) split launches, (c) checkpoints
def _agree(cell, ref, got, what, worst):
    """(b): counts, codes and steps identical; complex path: every field bit for bit; real paths: us, xs within 1e-10 at every
    step and the final guesses within 1e-7 (worst: the largest of each seen)."""
    for f in ("qp_solves", "exit_codes", "steps_done"):
        assert np.array_equal(got[f], ref[f]), (what, f, got[f], ref[f])
    if cell.path == kv.COMPLEX:
        for f in ("xs", "us", "x_guess", "u_guess"):
            assert _same(got[f], ref[f]), (what, f)
        return
    e_out = max(max(rel(got["us"][:, k], ref["us"][:, k]) for k in range(NS)),
                max(rel(got["xs"][:, k], ref["xs"][:, k]) for k in range(NS + 1)))
    e_guess = max(rel(got["x_guess"], ref["x_guess"]), rel(got["u_guess"], ref["u_guess"]))
    worst[0], worst[1] = max(worst[0], e_out), max(worst[1], e_guess)
    assert e_out <= 1e-10 and e_guess <= 1e-7, (what, e_out, e_guess)


@pytest.mark.parametrize("cell", PLANT_CELLS, ids=kv.cell_id)
def test_split_launches_and_checkpoints_match_one_launch(cell, record_property):
    """(b) run(k, k + 1) for k = 0..13, and run(0, k) + run(k, 14) at and beside every cut, on the session of the one launch, against
    it; (c) state() after run(0, k), k = 2, 7, restored (with the QP-solve counts) into a fresh session and run(k, 14) there: the
    same-session resume bit for bit on every path - anything else reads device state a checkpoint does not hold."""
    p = _scenario(cell)
    B = p["batch"]
    worst = [0.0, 0.0]
    resumed, checkpoints = {}, {}
    sess = _open(cell, p)
    try:
        assert sess.path_detail() == cell.path
        sess.run(0, NS)
        ref = _snapshot(sess)
        assert np.all(ref["exit_codes"] == 0) and np.all(ref["steps_done"] == NS)
        for k in range(NS):
            sess.run(k, k + 1)
        _agree(cell, ref, _snapshot(sess), "single steps", worst)
        for k in RESUME_AT:
            sess.run(0, k)
            if k in CHECKPOINT_AT:
                checkpoints[k] = (sess.state(), sess.download(_lib.F_QP_SOLVES, (B, NS)))
            sess.run(k, NS)
            resumed[k] = _snapshot(sess)
            _agree(cell, ref, resumed[k], "resumed at %d" % k, worst)
        assert sess.path_detail() == cell.path
    finally:
        sess.close()
    record_property("split_max_rel", worst)
    for k in CHECKPOINT_AT:
        st, solves = checkpoints[k]
        fresh = _open(cell, p)
        try:
            fresh.restore(st)
            fresh.upload(_lib.F_QP_SOLVES, solves)
            fresh.run(k, NS)
            got = _snapshot(fresh)
            assert fresh.path_detail() == cell.path
        finally:
            fresh.close()
        for f in got:
            assert _same(got[f], resumed[k][f]), (k, f)


# ---------------------------------------------------------------- (d) placement and row reuse
def _big_batch(cell, p5):
    """BIG members: the five of p5 at first index, the last full wavefront, the final partial one and the last index, and each at
    two drawn positions (one among the last heads); fillers from a larger draw of the same scenario (its first five left out: they
    repeat p5's), spread initial states, their own model scales or detunings.  One filler has a non-finite model (a NaN scale
    on the shared-generator path) where models are per member.  Returns (inputs, positions [5, 4], non-finite member or None)."""
    rng = np.random.default_rng(4099)
    pb = _take(_scenario(cell, batch=BIG + kv.BATCH), np.arange(kv.BATCH, BIG + kv.BATCH))
    if cell.plant == kv.PROCESS:
        # (one shared initial process vector in the scenario: the fillers start from their own)
        for i in range(BIG):
            V = rx(1e-3 + 0.05 * rng.standard_normal())
            pb["x0"][i] = np.kron(V, V.conj()).reshape(-1)
    fixed = np.array([0, BIG - 4, BIG - 3, BIG - 2, BIG - 1])
    drawn = rng.choice(np.arange(1, BIG - LATE), kv.BATCH, replace=False)
    late = rng.choice(np.arange(BIG - LATE, BIG - 4), kv.BATCH, replace=False)
    pos = np.stack([fixed, drawn, late], axis=1)
    for key in PER_MEMBER:
        v5 = p5.get(key)
        if v5 is not None and len(v5) == kv.BATCH:
            for b in range(kv.BATCH):
                pb[key][pos[b]] = v5[b]
    fill = np.setdiff1d(np.arange(BIG), pos.ravel())
    bad = None
    if cell.path == kv.SG:
        bad = int(fill[7])
        pb["scales"][bad, 0] = np.nan
    elif pb["models"].shape[0] > 1:
        bad = int(fill[7])
        pb["models"][bad] = np.nan
    return pb, pos, bad


@pytest.mark.parametrize("cell", PLANT_CELLS, ids=kv.cell_id)
def test_placement_and_row_reuse_bit_identical(cell, monkeypatch):
    """The five members, each at four places of a batch of 4,099 on a grid of one workgroup per CU (M4Q_WGS_PER_CU=1: every row
    runs four members or more, the pieces of a member on different rows), among fillers of which one fails at step 0 (code 3)
    and 42 exit (code 1, QuadraticExit on their own stored state) at steps 0..13 - every piece; and members 0 and 4 alone (B = 1:
    one active row, three idle).  Every copy equals the B = 5 launch bit for bit, guesses included, with and without the exits;
    the fillers' exits land where planned (_check_planned)."""
    monkeypatch.setenv("M4Q_WGS_PER_CU", "1")
    p5 = _scenario(cell)
    ref = _reference(cell, p5)
    pb, pos, bad = _big_batch(cell, p5)
    n = pb["dim_x"]

    def copies_equal(got, what):
        for b in range(kv.BATCH):
            for i in pos[b]:
                for f in ref:
                    assert _same(got[f][i], ref[f][b]), (what, b, int(i), f)

    sess = _open(cell, pb)
    try:
        assert sess.path_detail() == cell.path
        grid = sess.info()["grid"]
        assert BIG >= 16 * grid, (BIG, grid)
        sess.run(0, NS)
        free = _snapshot(sess)
        copies_equal(free, "no exits")
        keep = np.ones(BIG, dtype=bool)
        if bad is not None:
            assert free["exit_codes"][bad] == 3 and free["steps_done"][bad] == 0
            keep[bad] = False
        assert np.all(free["exit_codes"][keep] == 0) and np.all(free["steps_done"][keep] == NS)
        # fillers that exit: the state their planned step stores ('next': xs[k + 1]); nobody else ever meets its target
        fill = np.setdiff1d(np.flatnonzero(keep), pos.ravel())
        exiting = fill[11::97][:3 * NS]
        steps = np.full(BIG, NS)
        steps[exiting] = np.arange(len(exiting)) % NS
        target = _planned(free["xs"], "next", NS, steps=steps)
        sess.set_exit_condition(m4q.QuadraticExit(np.identity(n), target, 1e-30, state="next", fires="below"))
        sess.run(0, NS)
        got = _snapshot(sess)
        assert sess.path_detail() == cell.path
    finally:
        sess.close()
    copies_equal(got, "with exits")
    if bad is not None:
        assert got["exit_codes"][bad] == 3 and got["steps_done"][bad] == 0
    _check_planned({f: free[f][keep] for f in OUTPUTS}, {f: got[f][keep] for f in OUTPUTS}, target[keep], "next", NS)
    assert np.sum(got["exit_codes"] == 1) == len(exiting) == 3 * NS
    assert np.array_equal(got["steps_done"][exiting], steps[exiting])
    for b in (0, kv.BATCH - 1):
        one = _open(cell, _take(p5, [b]), model_per_instance=p5["models"].shape[0] > 1)
        try:
            assert one.path_detail() == cell.path
            one.run(0, NS)
            alone = _snapshot(one)
        finally:
            one.close()
        for f in ref:
            assert _same(alone[f][0], ref[f][b]), ("B = 1", b, f)


# ---------------------------------------------------------------- (e) exits across the exact pieces
@pytest.mark.parametrize("cell", [c for c in PLANT_CELLS if c.exact], ids=kv.cell_id)
def test_planned_exits_across_the_exact_pieces(cell):
    """Ten members, one planned exit each at EXIT_STEPS - in all five pieces of the exact launch, at and beside the cuts: code 1
    and steps_done exactly there, the run up to it bit-identical to the run without a condition; 'prev' and 'next'; cleared,
    the run without a condition again."""
    p = _scenario(cell, batch=len(EXIT_STEPS))
    n = p["dim_x"]
    sess = _open(cell, p)
    try:
        assert sess.path_detail() == cell.path
        sess.run(0, NS)
        ref = sess.results()
        assert np.all(ref["exit_codes"] == 0) and np.all(ref["steps_done"] == NS)
        for state in ("prev", "next"):
            target = _planned(ref["xs"], state, NS, steps=EXIT_STEPS)
            sess.set_exit_condition(m4q.QuadraticExit(np.identity(n), target, 1e-30, state=state, fires="below"))
            sess.run(0, NS)
            got = sess.results()
            _check_planned(ref, got, target, state, NS)
            assert np.all(got["exit_codes"] == 1) and np.array_equal(got["steps_done"], EXIT_STEPS), (state, got["steps_done"])
        sess.set_exit_condition(None)
        sess.run(0, NS)
        again = sess.results()
    finally:
        sess.close()
    for f in OUTPUTS:
        assert _same(again[f], ref[f]), f

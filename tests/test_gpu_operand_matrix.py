"""Every closed-loop kernel variant with moving and per-member operands (-m gpu).

tests/test_gpu_variant_matrix.py runs every cell of kernel_variants.closed_loop_cells() on one operand layout: a target constant
over the window and shared by the members, a shared plant (the process cells aside), per-member models.  The two families of
tests/operand_cases.py move what that layout holds still - "per": per-member constant targets, control targets and plant
operators, every stride of mpc_kernel non-zero; "moving": one moving target, one model, one plant, every stride zero - and each
(cell, family) is one teacher-forced case here, held to the oracle at the variant matrix's fixed bounds by the variant matrix's
own loop (_teacher_forced).  There is no sensitivity clause and no admissions file: tests/test_operand_cases_host.py asserts on
the CPU that the oracle determines every step of every scenario to a tenth of these bounds, and that a kernel reading another
member's operand, or holding the target still, would miss them by four orders of magnitude.

The "per" cases run once more free: one launch of the five members against five B = 1 sessions that are given member b's model,
targets and plant as the SHARED operands - bit for bit, on every path, which catches a stride error however small its effect.

A tile cell under the moving family is opened as a tile cell and must report 'traceless' (the tile sweep takes a constant target
only); test_tile_sessions_fall_back_on_a_moving_target asserts both directions of that decision on one session.

Rule-based exceptions, by name: none of the (cell, family) cases is skipped.  The shared-generator cells keep per-member scales
in the moving family and in the B = 1 sessions (that kernel has no shared-model form: m4q_session_build_models refuses scales
without model_per_instance), and PLANT_NONE cells run the free comparison step by step, each state handed over by put_state."""
import numpy as np
import pytest

from mpc4quantum_amd import _lib
from tests import kernel_variants as kv
from tests import operand_cases as oc
from tests.test_gpu_launch_schedule import _same, _snapshot
from tests.test_gpu_variant_matrix import _open, _teacher_forced

pytestmark = pytest.mark.gpu

CELLS = kv.closed_loop_cells()
CASES = [(c, f) for c in CELLS for f in oc.FAMILIES]


def _case_id(case):
    return "%s-%s" % (kv.cell_id(case[0]), case[1])


def _layout(p, **over):
    kw = dict(model_per_instance=p["model_per"], target_per_instance=p["target_per"], plant_per_instance=p["plant_per"])
    kw.update(over)
    return kw


def test_cells_that_leave_their_constant_target_code_only_here(capsys):
    """The list of record: the cells whose general sweep and rollout (clipped, kv.has_tc), moving-target pinned sweep (exact, the
    real paths) or fall-back (tile) run under the moving family and under no constant-target test."""
    only = [kv.cell_id(c) for c in CELLS if oc.only_through_moving(c)]
    with capsys.disabled():
        print("\n%d of %d closed-loop cells reach their moving-target code through the moving family:" % (len(only), len(CELLS)))
        for i in range(0, len(only), 6):
            print("  " + "  ".join(only[i:i + 6]))
    assert "9-2-1-traceless-clip-hamiltonian" in only and "9-2-1-real-exact-generator" in only


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_operand_family_teacher_forced(case, record_property):
    """One (cell, family): the variant matrix's teacher-forced loop on the family's scenario.  The session reports the expected
    path (the cell's own; 'traceless' for a tile cell with a moving target) before the first run and after the last; exit codes 0,
    identical QP-solve counts; clipped: us[k], xs[k+1] to 1e-10 relative, the guesses to 1e-7; exact: us[k] within 1e-9 of the
    bound, xs[k+1] within 1e-9; |u| <= sat (1 + 1e-15)."""
    cell, family = case
    run = oc.oracle(cell, family)
    p = run[0]
    us_got, _, worst = _teacher_forced(cell, run, path=oc.expected_path(cell, family), **_layout(p))
    record_property("worst_error_over_bound", worst)
    print("%s: worst error over bound %.3g" % (_case_id(case), worst))
    assert np.abs(us_got).max() <= p["sat"] * (1 + 1e-15)


def _free_run(cell, p, xs_t, **kw):
    """run(0, STEPS) of scenario p in one launch (PLANT_NONE: step by step, the state of each step from the oracle's run xs_t
    through put_state), and what it leaves behind."""
    sess = _open(cell, p, **kw)
    try:
        assert sess.path_detail() == cell.path
        if cell.plant == kv.NONE:
            for k in range(p["n_steps"]):
                sess.put_state(k, xs_t[:, k])
                sess.run(k, k + 1)
        else:
            sess.run(0, p["n_steps"])
        out = _snapshot(sess)
        assert sess.path_detail() == cell.path
    finally:
        sess.close()
    return out


@pytest.mark.parametrize("cell", CELLS, ids=kv.cell_id)
def test_member_alone_equals_its_row_of_the_batch(cell):
    """The "per" scenario free-running: one launch of the five members, every stride non-zero, against five B = 1 sessions that
    hold member b's model, target, control target and plant as shared operands (stride 0).  xs, us, qp_solves, x_guess, u_guess,
    exit_codes and steps_done of the member alone equal its row of the batch bit for bit."""
    p, xs_t = oc.oracle(cell, oc.PER)[:2]
    batch = _free_run(cell, p, xs_t, **_layout(p))
    assert np.all(batch["exit_codes"] == 0) and np.all(batch["steps_done"] == p["n_steps"])
    assert len({tuple(s) for s in batch["qp_solves"]}) > 1                  # the members do differ
    for b in range(p["batch"]):
        q = oc.member(p, b)
        alone = _free_run(cell, q, xs_t[b:b + 1], **_layout(q, model_per_instance=cell.path == kv.SG))
        for f in batch:
            assert _same(alone[f][0], batch[f][b]), (b, f)


@pytest.mark.parametrize("cell", [c for c in CELLS if c.path == kv.TILE], ids=kv.cell_id)
def test_tile_sessions_fall_back_on_a_moving_target(cell):
    """supported[PATH_TILE] = traceless && targ_const: a tile-allowed session with a moving target reports 'traceless', before and
    after a launch; the same session given the target's first column in every column reports 'traceless-tile', and back."""
    p = oc.scenario_of(cell, oc.MOVING)
    X = p["X_targ"]
    held = np.tile(X[:, :1], (1, X.shape[1]))
    sess = _open(cell, p, **_layout(p))
    try:
        assert sess.path_detail() == kv.TRACELESS
        sess.run(0, 1)
        assert sess.path_detail() == kv.TRACELESS and np.all(sess.state()["exit_codes"] == 0)
        sess.upload(_lib.F_X_TARG, held.T)
        assert sess.path_detail() == kv.TILE
        sess.run(0, 1)
        assert sess.path_detail() == kv.TILE and np.all(sess.state()["exit_codes"] == 0)
        sess.upload(_lib.F_X_TARG, X.T)
        assert sess.path_detail() == kv.TRACELESS
    finally:
        sess.close()

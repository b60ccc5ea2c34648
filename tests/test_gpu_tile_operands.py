"""The clipped tile sweep's operands through its LDS image (-m gpu): one launch run(0, 3) per case of tests/tile_operand_cases.py -
the three tile shapes on the TILE path, horizons 2, 3, 4 (a lone peeled block), 5, 6, 8 (a first block of 1, 2, 4 indices and the
peeled one), 9 (two blocks in the loop) and 40, five members and three.

Each case is held to the oracle's free run of the same scenario at the variant matrix's per-step bounds (QP-solve counts
identical, xs and us to 1e-10 relative, the guess left behind to 1e-7) and, byte for byte, to the library that selected and moved
the operands between lanes: SHA-256 of xs, us, qp_solves, x_guess and u_guess recorded from that build by
tools/record_tile_operands.py (tests/golden/tile_operand_checksums.json).  The image moves data only - the same products and sums
in the same order - so nothing but equality is accepted, and a case without a record fails.  The workgroup's LDS, the image
included, must stay at or under the eighth of a CU's 160 KB that eight workgroups per CU leave each."""
import json
import os

import numpy as np
import pytest

from oracle import m4q_oracle as orc
from tests import tile_operand_cases as tc

pytestmark = pytest.mark.gpu

RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_operand_checksums.json")

_ORACLE = {}


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


def _oracle(case):
    """The oracle's run of the case's scenario (cached: the two checks of a case share it)."""
    if case not in _ORACLE:
        p = tc.scenario(case)
        trace = []
        xs, us, codes, solves = orc.mpc_batch(p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], p["dt"],
                                              p["horizon"], p["n_steps"], p["plant_op0"], list(p["plant_ops"][0]), p["Q"], p["R"],
                                              p["Qf"], p["sat"], p["du"], qp_mode="qp", trace=trace)
        B = p["batch"]
        _ORACLE[case] = (p, np.swapaxes(xs, 1, 2), np.swapaxes(us, 1, 2), codes, solves,
                         np.stack([trace[b][-1][0].T for b in range(B)]), np.stack([trace[b][-1][1].T for b in range(B)]))
    return _ORACLE[case]


@pytest.fixture(scope="module")
def records():
    with open(RECORDS) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs():
    """One device run per case, shared by the two checks."""
    done = {}

    def run(case):
        if case not in done:
            done[case] = tc.run_case(case, _oracle(case)[0])
        return done[case]
    return run


def test_blocks_of_the_horizons():
    assert [tc.blocks(T) for T in tc.HORIZONS] == [[2], [3], [4], [1, 4], [2, 4], [4, 4], [1, 4, 4], [4] * 10]


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_against_the_oracle(case, runs):
    p, xs_t, us_t, codes, solves, xg_t, ug_t = _oracle(case)
    assert np.all(codes == 0)
    got = runs(case)
    figures = {"us": rel(got["us"], us_t), "xs": rel(got["xs"], xs_t), "x_guess": rel(got["x_guess"], xg_t),
               "u_guess": rel(got["u_guess"], ug_t)}
    print(tc.case_id(case), {k: float("%.3g" % v) for k, v in figures.items()}, "solves", got["qp_solves"].tolist())
    assert np.all(got["exit_codes"] == 0) and np.all(got["steps_done"] == tc.STEPS)
    assert np.array_equal(got["qp_solves"], solves)
    assert max(figures["us"], figures["xs"]) <= 1e-10, figures
    assert max(figures["x_guess"], figures["u_guess"]) <= 1e-7, figures
    assert np.abs(got["us"]).max() <= p["sat"] * (1 + 1e-15)


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_bit_identical_to_lane_moves(case, runs, records):
    name = tc.case_id(case)
    assert name in records, "no record for %s: run tools/record_tile_operands.py on the build without the image" % name
    assert tc.checksums(runs(case)) == records[name]


@pytest.mark.parametrize("cell", tc.CELLS, ids=lambda c: "%d_%d_%d" % (c.nx, c.nu, c.order))
def test_workgroup_lds_keeps_eight_per_cu(cell):
    """What the session allocates per workgroup on the TILE path, the image included: at or under an eighth of a CU's 160 KB."""
    import mpc4quantum_amd as m4q
    from tests import kernel_variants as kv
    p = tc.scenario(tc.Case(cell, 2, 3))
    sess = m4q.EnsembleSession(p["batch"], p["dim_x"], p["dim_u"], p["order"], p["horizon"], p["n_steps"], p["dt"], p["sat"], p["du"],
                               plant_kind=kv.PLANT_CODE[cell.plant], model_per_instance=p["models"].shape[0] > 1,
                               target_cols=p["n_steps"] + p["horizon"] + 1, force_complex=False, traceless=True, tile=True,
                               shared_generators=False, exact_qp=False)
    try:
        sess.load_problem(p["models"], p["x0"], p["X_targ"], p["U_targ"], p["Q"], p["R"], p["Qf"], p["plant_op0"], p["plant_ops"])
        sess.run(0, 1)                       # (the launch settles which kernel the session runs)
        assert sess.path_detail() == kv.TILE
        info = sess.info()
    finally:
        sess.close()
    print(info)
    assert 0 < info["lds_bytes"] <= 20480, info

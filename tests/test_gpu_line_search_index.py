"""The line search's tabled node weights (-m gpu): one launch run(0, 3) of five members per case of
tests/line_search_index_cases.py - shape (9, 2, 1), traceless; steps 0 and 1 iterate the SQP and run the line search - at horizons
3, 15, 16 and 17 (one trip of the nodes loop, and the second with one and two live lanes), 40 (the workload's), 46 and 47 (the last
tabled horizon of the tile kernel and the first without the table), on the tile kernel and, with M4Q_NO_TILE=1, on the DPP rows.

Each case is held, bit for bit, to the library whose line search formed every weight from its Z slot: SHA-256 of xs, us, x_guess, u_guess,
the exit codes and qp_solves recorded from that build by tools/record_line_search.py (tests/golden/line_search_index.json; a case
without a record fails) - and to the oracle's free run of the same scenario at the bounds of tests/test_gpu_guess_shift.py for a
clipped solve: QP-solve counts identical, xs and us to 1e-10 relative, the guess left behind to 1e-7."""
import json
import os

import numpy as np
import pytest

from oracle import m4q_oracle as orc
from tests import line_search_index_cases as lc

pytestmark = pytest.mark.gpu

RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_search_index.json")

_ORACLE = {}


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


def _oracle(case):
    """The oracle's run of the case's scenario (cached: both kernels of one horizon share it)."""
    key = case.horizon
    if key not in _ORACLE:
        p = lc.scenario(case)
        trace = []
        xs, us, codes, solves = orc.mpc_batch(p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], p["dt"],
                                              p["horizon"], p["n_steps"], p["plant_op0"], list(p["plant_ops"][0]), p["Q"], p["R"],
                                              p["Qf"], p["sat"], p["du"], qp_mode="qp", trace=trace)
        B = p["batch"]
        _ORACLE[key] = (p, np.swapaxes(xs, 1, 2), np.swapaxes(us, 1, 2), codes, solves,
                        np.stack([trace[b][-1][0].T for b in range(B)]), np.stack([trace[b][-1][1].T for b in range(B)]))
    return _ORACLE[key]


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
            done[case] = lc.run_case(case, _oracle(case)[0])
        return done[case]
    return run


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_against_the_oracle(case, runs):
    p, xs_t, us_t, codes, solves, xg_t, ug_t = _oracle(case)
    assert np.all(codes == 0)
    assert solves[:, :2].min() >= 2 and np.all(solves[:, 2] == 1)          # the line search runs on steps 0 and 1; then a warm step
    got = runs(case)
    sat = p["sat"]
    figures = {"us": rel(got["us"], us_t), "xs": rel(got["xs"], xs_t), "x_guess": rel(got["x_guess"], xg_t),
               "u_guess": rel(got["u_guess"], ug_t)}
    print(lc.case_id(case), {k: float("%.3g" % v) for k, v in figures.items()}, "solves", got["qp_solves"].tolist())
    assert np.all(got["exit_codes"] == 0) and np.all(got["steps_done"] == lc.STEPS)
    assert np.array_equal(got["qp_solves"], solves)
    assert max(figures["us"], figures["xs"]) <= 1e-10, figures
    assert max(figures["x_guess"], figures["u_guess"]) <= 1e-7, figures
    assert np.abs(got["us"]).max() <= sat * (1 + 1e-15)


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_bit_identical_to_the_untabled_line_search(case, runs, records):
    name = lc.case_id(case)
    assert name in records, "no record for %s: run tools/record_line_search.py on the build without the table" % name
    assert lc.checksums(runs(case)) == records[name]

"""The guess update that stores a finished step's guess one node down (-m gpu): one launch run(0, 3) of five members - two SQP
steps with all their iterations, then one warm step - per form of the update (tests/guess_shift_cases.py: X_guess in 16-byte pairs
or element by element, complex elements, U_guess in pairs or element by element, one exact kernel), at horizons where the
update's trips of loads-then-stores end at, before and after the end of the row's array.

Each case is held to the oracle's free run of the same scenario at the variant matrix's per-step bounds (clipped solve: QP-solve
counts identical, xs and us to 1e-10 relative, the guess left behind to 1e-7; exact solve: counts identical, us within 1e-9 of
the bound, xs within 1e-9, the guess to 1e-7) and, bit for bit, to the library that still updated and then shifted in a second
pass: SHA-256 of xs, us, qp_solves, x_guess and u_guess recorded from that build by tools/record_guess_shift.py
(tests/golden/guess_shift_checksums.json) - and, because the warm third step's rollout rewrites the whole guess, of the guess a
second launch run(0, 2) leaves: the shifted stores of step 1 themselves.  A case without a record fails."""
import json
import os

import numpy as np
import pytest

from oracle import m4q_oracle as orc
from tests import guess_shift_cases as gs
from tests import kernel_variants as kv

pytestmark = pytest.mark.gpu

RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guess_shift_checksums.json")

_ORACLE = {}


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


def _oracle(case):
    """The oracle's run of the case's scenario (cached: every path of one shape, solve and horizon shares it)."""
    c = case.cell
    key = (c.nx, c.nu, c.order, c.exact, case.horizon)
    if key not in _ORACLE:
        p = gs.scenario(case)
        trace = []
        xs, us, codes, solves = orc.mpc_batch(p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], p["dt"],
                                              p["horizon"], p["n_steps"], p["plant_op0"], list(p["plant_ops"][0]), p["Q"], p["R"],
                                              p["Qf"], p["sat"], p["du"], qp_mode="exact" if c.exact else "qp", trace=trace)
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

    def run(case, steps=gs.STEPS):
        if (case, steps) not in done:
            done[case, steps] = gs.run_case(case, _oracle(case)[0], steps)
        return done[case, steps]
    return run


@pytest.mark.parametrize("case", gs.CASES, ids=gs.case_id)
def test_against_the_oracle(case, runs):
    p, xs_t, us_t, codes, solves, xg_t, ug_t = _oracle(case)
    assert np.all(codes == 0)
    assert solves[:, :2].min() >= 2 and np.all(solves[:, 2] == 1)          # SQP iterations on steps 0 and 1, then a warm step
    got = runs(case)
    sat = p["sat"]
    figures = {"us": rel(got["us"], us_t), "xs": rel(got["xs"], xs_t), "x_guess": rel(got["x_guess"], xg_t),
               "u_guess": rel(got["u_guess"], ug_t), "us_abs/sat": np.abs(got["us"] - us_t).max() / sat,
               "xs_abs": np.abs(got["xs"] - xs_t).max()}
    print(gs.case_id(case), {k: float("%.3g" % v) for k, v in figures.items()}, "solves", got["qp_solves"].tolist())
    assert np.all(got["exit_codes"] == 0) and np.all(got["steps_done"] == gs.STEPS)
    assert np.array_equal(got["qp_solves"], solves)
    if case.cell.exact:
        assert figures["us_abs/sat"] <= 1e-9 and figures["xs_abs"] <= 1e-9, figures
    else:
        assert max(figures["us"], figures["xs"]) <= 1e-10, figures
    assert max(figures["x_guess"], figures["u_guess"]) <= 1e-7, figures
    assert np.abs(got["us"]).max() <= sat * (1 + 1e-15)


@pytest.mark.parametrize("case", gs.CASES, ids=gs.case_id)
def test_bit_identical_to_update_then_shift(case, runs, records):
    name = gs.case_id(case)
    assert name in records, "no record for %s: run tools/record_guess_shift.py on the two-pass build" % name
    assert gs.checksums(runs(case), runs(case, gs.SQP_STEPS)) == records[name]

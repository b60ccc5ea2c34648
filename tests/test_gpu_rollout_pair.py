"""The rollout's pair form at n = 8 (-m gpu): one launch run(0, 3) per case of tests/rollout_pair_cases.py - cell (9, 2, 1) on the
TILE and on the TRACELESS (DPP) path, horizons 1 (the upper half never live), 2 (one pair), 3 (a pair and an odd tail), 7 and 8,
five members and three, and one case with the du band on (the first index's box binds in the lower half of the first trip only).

Each case is held to the oracle's free run of the same scenario at the bounds of tests/test_gpu_tile_operands.py (QP-solve counts
identical, xs and us to 1e-10 relative, the guess left behind to 1e-7) and, byte for byte, to the library that rolled one index
at a time: SHA-256 of xs, us, qp_solves, x_guess and u_guess, recorded from that build by tools/record_rollout_pair.py
(tests/golden/rollout_pair_checksums.json) or, where the launch is one of theirs, by the tile-operand and guess-shift records.
The pair form moves work between lanes only - the same products and sums in the same order - so nothing but equality is
accepted, and a case without a record fails."""
import json
import os

import numpy as np
import pytest

from oracle import m4q_oracle as orc
from tests import rollout_pair_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_ORACLE = {}


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


def _oracle(case):
    """The oracle's run of the case's scenario (cached: the two checks of a case share it)."""
    if case not in _ORACLE:
        p = rc.scenario(case)
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
    out = {}
    for name in ("rollout_pair_checksums.json", "tile_operand_checksums.json", "guess_shift_checksums.json"):
        with open(os.path.join(GOLDEN, name)) as f:
            out[name] = json.load(f)
    return out


@pytest.fixture(scope="module")
def runs():
    """One device run per case, shared by the two checks."""
    done = {}

    def run(case):
        if case not in done:
            done[case] = rc.run_case(case, _oracle(case)[0])
        return done[case]
    return run


def test_records_are_not_duplicated(records):
    """A launch another file already records is read from there."""
    own = {rc.case_id(c) for c in rc.own_cases()}
    assert set(records["rollout_pair_checksums.json"]) == own
    shared = [c for c in rc.CASES if rc.case_id(c) not in own]
    assert shared and all(rc.record_of(c)[1] in records[rc.record_of(c)[0]] for c in shared)


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_against_the_oracle(case, runs):
    p, xs_t, us_t, codes, solves, xg_t, ug_t = _oracle(case)
    assert np.all(codes == 0)
    got = runs(case)
    figures = {"us": rel(got["us"], us_t), "xs": rel(got["xs"], xs_t), "x_guess": rel(got["x_guess"], xg_t),
               "u_guess": rel(got["u_guess"], ug_t)}
    print(rc.case_id(case), {k: float("%.3g" % v) for k, v in figures.items()}, "solves", got["qp_solves"].tolist())
    assert np.all(got["exit_codes"] == 0) and np.all(got["steps_done"] == rc.STEPS)
    assert np.array_equal(got["qp_solves"], solves)
    assert max(figures["us"], figures["xs"]) <= 1e-10, figures
    assert max(figures["x_guess"], figures["u_guess"]) <= 1e-7, figures
    assert np.abs(got["us"]).max() <= p["sat"] * (1 + 1e-15)
    if case.du is not None:
        # the band binds: some applied control sits a full band away from the one before it (the oracle's does)
        step = np.abs(np.diff(us_t, axis=1)).max()
        print("largest step of a control %.6g, band %.6g" % (step, p["du"]))
        assert step >= p["du"] * (1 - 1e-9)
        assert np.abs(np.diff(got["us"], axis=1)).max() <= p["du"] * (1 + 1e-12)


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_bit_identical_to_one_index_per_trip(case, runs, records):
    name, key, fields = rc.record_of(case)
    assert key in records[name], "no record for %s in %s: run tools/record_rollout_pair.py on the build before the pair form" % (key, name)
    sums = rc.checksums(runs(case))
    assert {f: sums[f] for f in fields} == {f: records[name][key][f] for f in fields}

"""Checksums of tests/test_gpu_guess_shift.py's cases from the library in use (M4Q_LIB, or the in-tree one), as JSON on stdout:

    M4Q_LIB=<library that updates, then shifts in a second pass> python tools/record_guess_shift.py > tests/golden/guess_shift_checksums.json

Deterministic: the cases, seeds and sizes are those of tests/guess_shift_cases.py; one launch run(0, 3) per case: SHA-256 of xs, us,
qp_solves, x_guess and u_guess; and one launch run(0, 2): SHA-256 of the guess the two SQP steps leave."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import guess_shift_cases as gs  # noqa: E402


def main():
    out = {}
    for case in gs.CASES:
        res = gs.run_case(case)
        assert not res["exit_codes"].any(), (gs.case_id(case), res["exit_codes"])
        sqp = gs.run_case(case, steps=gs.SQP_STEPS)
        assert not sqp["exit_codes"].any() and (sqp["steps_done"] == gs.SQP_STEPS).all(), gs.case_id(case)
        out[gs.case_id(case)] = gs.checksums(res, sqp)
        sys.stderr.write("%s solves %s\n" % (gs.case_id(case), res["qp_solves"].tolist()))
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()

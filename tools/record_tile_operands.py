"""Checksums of tests/test_gpu_tile_operands.py's cases from the library in use (M4Q_LIB, or the in-tree one), as JSON on stdout:

    M4Q_LIB=<library that spreads the sweep's operands with lane moves> python tools/record_tile_operands.py > tests/golden/tile_operand_checksums.json

Deterministic: the cases, seeds and sizes are those of tests/tile_operand_cases.py; one launch run(0, 3) per case: SHA-256 of xs, us,
qp_solves, x_guess and u_guess."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import tile_operand_cases as tc  # noqa: E402


def main():
    out = {}
    for case in tc.CASES:
        res = tc.run_case(case)
        assert not res["exit_codes"].any() and (res["steps_done"] == tc.STEPS).all(), (tc.case_id(case), res["exit_codes"])
        out[tc.case_id(case)] = tc.checksums(res)
        sys.stderr.write("%s solves %s\n" % (tc.case_id(case), res["qp_solves"].tolist()))
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()

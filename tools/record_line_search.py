"""Checksums of tests/test_gpu_line_search_index.py's cases from the library in use (M4Q_LIB, or the in-tree one), as JSON on stdout:

    M4Q_LIB=<library whose line search forms every weight from its Z slot> python tools/record_line_search.py > tests/golden/line_search_index.json

Deterministic: the cases, seeds and sizes are those of tests/line_search_index_cases.py; one launch run(0, 3) per case: SHA-256 of
xs, us, x_guess, u_guess, exit_codes and qp_solves."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import line_search_index_cases as lc  # noqa: E402


def main():
    out = {}
    for case in lc.CASES:
        res = lc.run_case(case)
        assert not res["exit_codes"].any() and (res["steps_done"] == lc.STEPS).all(), (lc.case_id(case), res["exit_codes"])
        out[lc.case_id(case)] = lc.checksums(res)
        sys.stderr.write("%s solves %s\n" % (lc.case_id(case), res["qp_solves"].tolist()))
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()

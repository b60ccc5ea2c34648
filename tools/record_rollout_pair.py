"""Checksums of tests/test_gpu_rollout_pair.py's own cases from the library in use (M4Q_LIB, or the in-tree one), as JSON on stdout:

    M4Q_LIB=<library whose rollout takes one horizon index at a time> python tools/record_rollout_pair.py > tests/golden/rollout_pair_checksums.json

Deterministic: the cases, seeds and sizes are those of tests/rollout_pair_cases.py; one launch run(0, 3) per case: SHA-256 of xs, us,
qp_solves, x_guess and u_guess.  Cases whose launch tests/golden/tile_operand_checksums.json or guess_shift_checksums.json already
holds are not recorded again (rollout_pair_cases.record_of)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import rollout_pair_cases as rc  # noqa: E402


def main():
    out = {}
    for case in rc.own_cases():
        p = rc.scenario(case)
        res = rc.run_case(case, p)
        assert not res["exit_codes"].any() and (res["steps_done"] == rc.STEPS).all(), (rc.case_id(case), res["exit_codes"])
        out[rc.case_id(case)] = rc.checksums(res)
        note = ""
        if case.du is not None:
            # how far the applied controls move per step against the band (the first step from U_targ[:, 0])
            us = np.asarray(res["us"])
            note = " us%s max|du|/band %.6f" % (us.shape, np.abs(np.diff(us, axis=1)).max() / p["du"])
        sys.stderr.write("%s solves %s%s\n" % (rc.case_id(case), res["qp_solves"].tolist(), note))
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()

"""The cases of tests/test_gpu_line_search_index.py and tools/record_line_search.py (no device, no _lib load at import).

The node-per-lane line search of the clipped traceless kernels at d = 3 (line_search_tl_nodes, csrc/m4q_mpc.h) reads, in the tile
kernel, its node weights from a table that holds 47 nodes (csrc/m4q_ls_table.h).  One launch run(0, 3) of five members per case -
steps 0 and 1 iterate the SQP and run the line search, step 2 is warm - at
    T = 3, 15       one trip of the nodes loop: 4 of a row's 16 lanes own a node, and all of them
    T = 16, 17      a second trip with one and two live lanes, the others reading the last node's row
    T = 40          the workload's horizon
    T = 46, 47      the last tabled horizon and the first that runs without the table
on the tile kernel and, with M4Q_NO_TILE=1 in the environment, on the DPP rows (whose line search has no table)."""
import hashlib
import os
from collections import namedtuple

import numpy as np

from tests import guess_shift_cases as gs
from tests import kernel_variants as kv

BATCH, STEPS = 5, 3
HORIZONS = (3, 15, 16, 17, 40, 46, 47)
FIELDS = ("xs", "us", "x_guess", "u_guess", "exit_codes", "qp_solves")
CELLS = tuple(kv.LoopCell(9, 2, 1, path, False, kv.HAMILTONIAN) for path in (kv.TILE, kv.TRACELESS))

Case = namedtuple("Case", "cell horizon")
CASES = tuple(Case(cell, T) for cell in CELLS for T in HORIZONS)


def case_id(c):
    return "%s-T%d" % (kv.cell_id(c.cell), c.horizon)


def scenario(case):
    c = case.cell
    return kv.scenario(c.nx, c.nu, c.order, batch=BATCH, horizon=case.horizon, n_steps=STEPS)


def run_case(case, p=None):
    """One launch run(0, STEPS) of the case's kernel; the DPP cases with M4Q_NO_TILE=1 set while the session exists."""
    before = os.environ.get("M4Q_NO_TILE")
    if case.cell.path == kv.TILE:
        os.environ.pop("M4Q_NO_TILE", None)
    else:
        os.environ["M4Q_NO_TILE"] = "1"
    try:
        return gs.run_case(gs.Case(case.cell, case.horizon), scenario(case) if p is None else p, STEPS)
    finally:
        if before is None:
            os.environ.pop("M4Q_NO_TILE", None)
        else:
            os.environ["M4Q_NO_TILE"] = before


def checksums(out):
    """SHA-256 of the bytes of every field of FIELDS (C order, the dtypes the session hands out)."""
    return {f: hashlib.sha256(np.ascontiguousarray(out[f]).tobytes()).hexdigest() for f in FIELDS}

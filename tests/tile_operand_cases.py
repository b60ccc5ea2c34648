"""The cases of tests/test_gpu_tile_operands.py and tools/record_tile_operands.py (no device, no _lib load at import).

The clipped tile sweep (csrc/m4q_tile3.h) takes the horizon in blocks of four indices - the first block the (T - 1) % 4 + 1 top
ones, the block that holds t = 0 peeled out of the loop - and hands every block's operands to its indices through an LDS image
(csrc/m4q_tile_opnd.h).  One launch run(0, 3) per case - two SQP steps with all their iterations, then one warm step - on the TILE
path of each of the three tile shapes, at horizons that give
    T = 2, 3, 4     a lone peeled block of 2, 3 and 4 indices
    T = 5, 6, 8     a first block of 1, 2 and 4 indices, then the peeled full block
    T = 9           a partial block and a full one in the loop, then the peeled one
    T = 40          the workload's own horizon
with 5 members (a full wavefront and one more row: three members of the second wavefront are idle) and with 3."""
import hashlib
from collections import namedtuple

import numpy as np

from tests import guess_shift_cases as gs
from tests import kernel_variants as kv

STEPS = gs.STEPS
FIELDS = gs.FIELDS
HORIZONS = (2, 3, 4, 5, 6, 8, 9, 40)
BATCHES = (5, 3)
CELLS = tuple(kv.LoopCell(nx, nu, 1, kv.TILE, False, kv.HAMILTONIAN) for nx, nu in ((4, 1), (4, 2), (9, 2)))

Case = namedtuple("Case", "cell horizon batch")
CASES = tuple(Case(cell, T, B) for cell in CELLS for T in HORIZONS for B in BATCHES)


def case_id(c):
    return "%s-T%d-B%d" % (kv.cell_id(c.cell), c.horizon, c.batch)


def blocks(T):
    """Index counts of the sweep's blocks, top of the horizon first; the last one is the peeled block."""
    out = [(T - 1) % 4 + 1]
    while sum(out) < T:
        out.append(4)
    return out


def scenario(case):
    c = case.cell
    return kv.scenario(c.nx, c.nu, c.order, batch=case.batch, horizon=case.horizon, n_steps=STEPS)


def run_case(case, p=None):
    """One launch run(0, STEPS) of the case's kernel: the outputs and the guess it leaves, as arrays."""
    return gs.run_case(gs.Case(case.cell, case.horizon), scenario(case) if p is None else p, STEPS)


def checksums(out):
    """SHA-256 of the bytes of every field of FIELDS (C order, the dtypes the session hands out)."""
    return {f: hashlib.sha256(np.ascontiguousarray(out[f]).tobytes()).hexdigest() for f in FIELDS}

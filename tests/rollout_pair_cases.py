"""The cases of tests/test_gpu_rollout_pair.py and tools/record_rollout_pair.py (no device, no _lib load at import).

At n = 8 (the traceless coordinates of d = 3) the clipped forward rollout takes two horizon indices per trip, index 2 p on lanes
0..7 of the row and 2 p + 1 on lanes 8..15 (rollout_forward_pair in csrc/m4q_mpc.h, the map in csrc/m4q_rollout_pair.h).  One
launch run(0, 3) per case - two SQP steps with all their iterations, whose rows store to the solution arrays, then one warm step,
whose rows store into the shifted guess - on the TILE and the TRACELESS (DPP) path of cell (9, 2, 1), Hamiltonian plant, at
    T = 1       one index: the upper half never live
    T = 2       one pair
    T = 3       a pair and an odd tail
    T = 7, 8    the peeled first pair, the loop, a lone pair, with and without the tail
with 5 members (a full wavefront and one more row) and with 3; and one case with the du band on, so that the first index's
narrower box binds - in the lower half of the first trip only."""
from collections import namedtuple

from tests import guess_shift_cases as gs
from tests import kernel_variants as kv
from tests import tile_operand_cases as tc

STEPS = gs.STEPS
FIELDS = gs.FIELDS
HORIZONS = (1, 2, 3, 7, 8)
BATCHES = (5, 3)
CELLS = tuple(kv.LoopCell(9, 2, 1, path, False, kv.HAMILTONIAN) for path in (kv.TILE, kv.TRACELESS))
DU_BAND = 0.05                 # the du case: the band's half width in units of sat

Case = namedtuple("Case", "cell horizon batch du")
CASES = tuple(Case(cell, T, B, None) for cell in CELLS for T in HORIZONS for B in BATCHES) + (Case(CELLS[0], 7, 5, DU_BAND),)


def case_id(c):
    return "%s-T%d-B%d%s" % (kv.cell_id(c.cell), c.horizon, c.batch, "" if c.du is None else "-du")


def record_of(c):
    """(file under tests/golden, key, fields) of the case's record: the tile-operand and guess-shift records where they hold the
    same launch, this test's own file otherwise."""
    if c.du is None and c.cell.path == kv.TILE and c.horizon in tc.HORIZONS and c.batch in tc.BATCHES:
        return "tile_operand_checksums.json", tc.case_id(tc.Case(c.cell, c.horizon, c.batch)), FIELDS
    shift_case = gs.Case(c.cell, c.horizon)
    if c.du is None and c.batch == gs.BATCH and shift_case in gs.CASES:
        return "guess_shift_checksums.json", gs.case_id(shift_case), FIELDS
    return "rollout_pair_checksums.json", case_id(c), FIELDS


def own_cases():
    return tuple(c for c in CASES if record_of(c)[0] == "rollout_pair_checksums.json")


def scenario(case):
    c = case.cell
    p = kv.scenario(c.nx, c.nu, c.order, batch=case.batch, horizon=case.horizon, n_steps=STEPS)
    if case.du is not None:
        p["du"] = case.du * p["sat"]
    return p


def run_case(case, p=None):
    """One launch run(0, STEPS) of the case's kernel: the outputs and the guess it leaves, as arrays."""
    return gs.run_case(gs.Case(case.cell, case.horizon), scenario(case) if p is None else p, STEPS)


checksums = tc.checksums

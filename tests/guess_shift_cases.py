"""The cases of tests/test_gpu_guess_shift.py and tools/record_guess_shift.py, and the NumPy model of the store rule that
tests/test_guess_shift_host.py checks (no device, no _lib load at import).

mpc_kernel's guess update (X_guess += alpha (X_opt - X_guess), mpc.py:228-229) stores a row that ends its MPC step one node
down, so that no second pass shifts the guess (shift_guess, mpc.py:71-73): element e of the updated array of `nodes` nodes of
width w goes to e - w where e >= w and, the last node repeated, also to e where e >= (nodes - 1) w; node 0 is dropped.  The
update runs in batches of elements (all loads of a batch before its first store) in four forms - X_guess in 16-byte pairs
(real paths, n even) or element by element, U_guess likewise - and the horizons below sit where a batch ends at, before and
after the array's end."""
import hashlib
from collections import namedtuple

import numpy as np

from tests import kernel_variants as kv

BATCH, STEPS = 5, 3           # a full wavefront of four rows and one more row; two SQP steps with all their iterations, one warm step
FIELDS = ("xs", "us", "qp_solves", "x_guess", "u_guess")
# the warm third step's rollout rewrites the whole guess, so a second launch run(0, 2) of every case shows the guess as the
# shifted stores of step 1 left it
SQP_STEPS = 2
SQP_FIELDS = ("x_guess", "u_guess")

# elements per trip of the update's loop over one row's array: 16 lanes x (2 x 6 | 12) for X_guess, 16 x (2 x 4 | 8) for U_guess
X_TRIP, U_TRIP = 192, 128

Case = namedtuple("Case", "cell horizon")

_H = kv.HAMILTONIAN
# (cell, horizons): one cell per form of the update
#   pair form at n = 8: (T + 1) 8 = 192 fills one trip exactly at T = 23; T = 24 opens a second trip with clamped tail loads, and
#   the store to e - n crosses the trip boundary; T = 40 is the workload's horizon
#   element form at n = 9 complex: 189 and 198 elements against trips of 192
#   element form at n = 3 and n = 15: T = 2 and the first T whose element count passes one trip
_PLAN = (
    (kv.LoopCell(9, 2, 1, kv.TILE, False, _H), (2, 23, 24, 40)),            # pairs for X_guess and U_guess, the headline kernel
    (kv.LoopCell(9, 2, 1, kv.TRACELESS, False, _H), (2, 23, 24, 40)),       # ... on DPP rows
    (kv.LoopCell(4, 1, 1, kv.TRACELESS, False, _H), (2, 64)),               # n = 3: X_guess element by element
    (kv.LoopCell(9, 2, 1, kv.COMPLEX, False, _H), (2, 20, 21)),             # complex elements
    (kv.LoopCell(16, 3, 1, kv.TRACELESS, False, _H), (2, 12)),              # n = 15, m = 3: U_guess element by element
    (kv.LoopCell(16, 3, 1, kv.TRACELESS, True, _H), (2, 12)),               # an exact kernel, both arrays element by element (its
                                                                            # oracle, BVLS, takes seconds here and a minute at n = 8)
)
CASES = tuple(Case(cell, T) for cell, hs in _PLAN for T in hs)


def case_id(c):
    return "%s-T%d" % (kv.cell_id(c.cell), c.horizon)


def state_width(cell):
    """Elements per node of the row's X_guess as the kernel holds it: n - 1 real traceless coordinates, else n."""
    return cell.nx - 1 if cell.path in (kv.TRACELESS, kv.TILE, kv.SG) else cell.nx


def shapes_covered():
    """(T, n, m) of every case, n as the kernel holds it."""
    return sorted({(c.horizon, state_width(c.cell), c.cell.nu) for c in CASES})


# ---------------------------------------------------------------- the store rule
def destinations(e, width, nodes, shift):
    """Where the update stores element e of a row's array (`nodes` nodes of `width` elements)."""
    if not shift:
        return [e]
    out = []
    if e >= width:
        out.append(e - width)
    if e >= (nodes - 1) * width:
        out.append(e)
    return out


def update_in_place(g, o, alpha, width, nodes, shift, lanes_elems, unroll):
    """The update loop as the kernel runs it on one row, in place on g: per trip, `unroll` groups in which each of the 16 lanes
    takes `lanes_elems` consecutive elements; a trip issues all its loads (groups past the end clamped to the last one) before
    its first store, and every store goes where destinations() says.  Returns g."""
    count = width * nodes
    per = 16 * lanes_elems
    for t0 in range(0, count, per * unroll):
        loaded = []
        for u in range(unroll):                       # all loads of the trip first
            for lane in range(16):
                e0 = t0 + u * per + lane * lanes_elems
                src = e0 if e0 < count else count - lanes_elems
                loaded.append((e0, g[src:src + lanes_elems].copy(), o[src:src + lanes_elems].copy()))
        for e0, xg, xo in loaded:                     # then the stores, batch by batch
            if e0 >= count:
                continue
            r = xg + alpha * (xo - xg)
            for h in range(lanes_elems):
                for d in destinations(e0 + h, width, nodes, shift):
                    g[d] = r[h]
    return g


def update_then_shift(g, o, alpha, width, nodes):
    """The two passes the store rule replaces: the update, then shift_guess on [width, nodes] columns."""
    from mpc4quantum_amd.mpc import shift_guess
    r = g + alpha * (o - g)
    return shift_guess(r.reshape(nodes, width).T).T.reshape(-1)


# ---------------------------------------------------------------- running a case on the device
def scenario(case):
    c = case.cell
    return kv.scenario(c.nx, c.nu, c.order, batch=BATCH, horizon=case.horizon, n_steps=STEPS)


def run_case(case, p=None, steps=STEPS):
    """One launch run(0, steps) of the case's kernel: the outputs and the guess it leaves, as arrays."""
    import mpc4quantum_amd as m4q
    from mpc4quantum_amd import _lib
    cell = case.cell
    p = scenario(case) if p is None else p
    B, n, m = p["batch"], p["dim_x"], p["dim_u"]
    sess = m4q.EnsembleSession(B, n, m, p["order"], p["horizon"], p["n_steps"], p["dt"], p["sat"], p["du"],
                               plant_kind=kv.PLANT_CODE[cell.plant], model_per_instance=p["models"].shape[0] > 1,
                               target_cols=p["n_steps"] + p["horizon"] + 1, force_complex=cell.path == kv.COMPLEX,
                               traceless=cell.path != kv.REAL, tile=cell.path == kv.TILE, shared_generators=False,
                               exact_qp=cell.exact)
    try:
        sess.load_problem(p["models"], p["x0"], p["X_targ"], p["U_targ"], p["Q"], p["R"], p["Qf"], p["plant_op0"], p["plant_ops"])
        assert sess.path_detail() == cell.path, (sess.path_detail(), cell.path)
        sess.run(0, steps)
        st = sess.state()
        out = {"xs": st["xs"], "us": st["us"], "x_guess": st["x_guess"], "u_guess": st["u_guess"],
               "qp_solves": sess.download(_lib.F_QP_SOLVES, (B, STEPS)), "exit_codes": st["exit_codes"],
               "steps_done": st["steps_done"]}
        assert sess.path_detail() == cell.path
    finally:
        sess.close()
    return out


def checksums(out, out_sqp):
    """SHA-256 of the bytes of every field of FIELDS of the run(0, STEPS) launch and, as <field>_after_sqp, of SQP_FIELDS of the
    run(0, SQP_STEPS) launch (C order, the dtypes the session hands out)."""
    sums = {f: hashlib.sha256(np.ascontiguousarray(out[f]).tobytes()).hexdigest() for f in FIELDS}
    sums.update({f + "_after_sqp": hashlib.sha256(np.ascontiguousarray(out_sqp[f]).tobytes()).hexdigest() for f in SQP_FIELDS})
    return sums

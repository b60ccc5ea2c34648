"""Results do not depend on what shares the SIMD (-m gpu).

The closed-loop kernels set the wavefront's issue priority by phase (m4q_kernels.hip: PrioMap), which changes how the two
wavefronts of a SIMD interleave and nothing else: no arithmetic instruction, no wait of one wavefront for another.  The placement
tests elsewhere run at M4Q_WGS_PER_CU=1 or at batches that leave SIMDs half empty; here five members run alone (B = 5: two
wavefronts on the whole device) and then at fixed positions of B = 8,192 + 3 - the first two drawn, one in the middle, one among
the last heads the queue hands out and the very last, whose wavefront is ragged - which is 2,048 resident wavefronts at the
default grid: both wavefronts of every SIMD busy, in different phases, tails polling for heads that other workgroups publish.
Every output and the guesses left behind are equal as bits, and every exit code is 0.

Shapes: config 3's (qutrit, n = 8 traceless coordinates, m = 2) and config 2's (qubit, n = 3, m = 1) at T = 5 - a block of one
index, then the peeled block of the tile sweep - and 4 steps: a head [0, 2) and a tail [2, 4) per member.  Every member starts
from a random pure state (config 3's own start is all but a stationary point of so short a horizon); the fillers are the other
members of the same draw."""
import functools

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import configs

pytestmark = pytest.mark.gpu

T = 5
STEPS = 4
BIG = 8192 + 3
POSITIONS = (0, 1, BIG // 2, BIG - 256, BIG - 1)       # first, middle, among the last heads drawn, the ragged last wavefront
OUTPUTS = ("xs", "us", "qp_solves", "exit_codes", "steps_done", "x_guess", "u_guess")
CFG_OF_D = {2: 2, 3: 3}
# (d, exact, tile): the clipped tile kernel, the DPP sweeps (M4Q_NO_TILE=1), the exact mode on tiles, the same at d = 2
CELLS = [(3, False, True), (3, False, False), (3, True, True), (2, False, True), (2, False, False), (2, True, True)]


def _same(a, b):
    """Identical bits (floating-point fields compared as integers: -0.0 is not 0.0, a NaN equals its own bits)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint64), b.view(np.uint64)) if a.dtype.kind in "fc" else np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def _problem(d):
    """BIG members of the configuration's draw, every one started from a random pure state (shared: callers do not modify it)."""
    p = configs.build(CFG_OF_D[d], batch=BIG, order=1, horizon=T, n_steps=STEPS)
    rng = np.random.default_rng(11)
    psi = rng.standard_normal((BIG, d)) + 1j * rng.standard_normal((BIG, d))
    psi /= np.linalg.norm(psi, axis=1, keepdims=True)
    p["x0"] = np.ascontiguousarray(np.einsum('bi,bj->bij', psi, psi.conj()).reshape(BIG, -1))
    for key in ("x0", "models"):
        p[key].setflags(write=False)
    return p


def _run(p, idx, exact):
    """One launch run(0, STEPS) of the members idx of p (None: all): outputs and the guesses left behind."""
    x0, models = p["x0"], p["models"]
    per_member = models.shape[0] > 1
    if idx is not None:
        x0 = np.ascontiguousarray(x0[list(idx)])
        if per_member:
            models = np.ascontiguousarray(models[list(idx)])
    B = x0.shape[0]
    sess = m4q.EnsembleSession(B, p["dim_x"], p["dim_u"], p["order"], T, STEPS, p["dt"], p["sat"], p["du"],
                               model_per_instance=per_member, target_cols=STEPS + T + 1, exact_qp=exact)
    try:
        sess.load_problem(models, x0, p["X_targ"], p["U_targ"], p["Q"], p["R"], p["Qf"], p["plant_op0"], p["plant_ops"])
        path = sess.path_detail()
        sess.run(0, STEPS)
        r, st = sess.results(), sess.state()
    finally:
        sess.close()
    out = {f: (r[f] if f in r else st[f]) for f in OUTPUTS}
    return path, out


@pytest.mark.parametrize("d,exact,tile", CELLS)
def test_members_alone_and_at_full_residency_agree_bit_for_bit(d, exact, tile, monkeypatch):
    if tile:
        monkeypatch.delenv("M4Q_NO_TILE", raising=False)
    else:
        monkeypatch.setenv("M4Q_NO_TILE", "1")
    monkeypatch.delenv("M4Q_WGS_PER_CU", raising=False)         # the default grid: two wavefronts on every SIMD
    p = _problem(d)
    want = "traceless-tile" if tile else "traceless"
    path_a, alone = _run(p, POSITIONS, exact)
    path_b, full = _run(p, None, exact)
    assert path_a == want and path_b == want, (path_a, path_b)
    assert np.all(full["exit_codes"] == 0) and np.all(full["steps_done"] == STEPS), \
        (np.unique(full["exit_codes"]), np.unique(full["steps_done"]))
    assert np.all(alone["exit_codes"] == 0)
    for f in OUTPUTS:
        got = full[f][list(POSITIONS)]
        assert _same(got, alone[f]), (f, [int(b) for b in range(len(POSITIONS)) if not _same(got[b], alone[f][b])])

"""The store rule of mpc_kernel's guess update on the host (no GPU): a NumPy model of the element -> destination map, with the
duplicate for the last node, run in place in the kernel's trips of loads-then-stores, against update-then-shift_guess
(mpc.py:228-229, then :71-73).  Every (T, n, m) of tests/test_gpu_guess_shift.py and T = 1."""
import numpy as np
import pytest

from tests import guess_shift_cases as gs

SHAPES = gs.shapes_covered()
SHAPES = SHAPES + sorted({(1, n, m) for _, n, m in SHAPES})


def _x_form(n, complex_elems):
    """(elements per lane, groups per trip) of the update of X_guess; _u_form: of U_guess."""
    return (2, 6) if n % 2 == 0 and not complex_elems else (1, 12)


def _u_form(m):
    return (2, 4) if m % 2 == 0 else (1, 8)


def _arrays(rng, count, complex_elems):
    g = rng.standard_normal(count)
    o = rng.standard_normal(count)
    if complex_elems:
        g = g + 1j * rng.standard_normal(count)
        o = o + 1j * rng.standard_normal(count)
    return g, o


def test_every_horizon_of_the_gpu_test_is_here_and_T_1():
    assert {(c.horizon, gs.state_width(c.cell), c.cell.nu) for c in gs.CASES} <= set(SHAPES)
    assert any(T == 1 for T, _, _ in SHAPES)
    # the horizons sit where the table of the GPU test says: one X trip filled exactly, one element group more, and below
    assert (23 + 1) * 8 == gs.X_TRIP and (24 + 1) * 8 > gs.X_TRIP
    assert (20 + 1) * 9 < gs.X_TRIP < (21 + 1) * 9
    assert (63 + 1) * 3 == gs.X_TRIP < (64 + 1) * 3 and (11 + 1) * 15 < gs.X_TRIP < (12 + 1) * 15


@pytest.mark.parametrize("T,n,m", SHAPES)
def test_destination_map_is_the_shift(T, n, m):
    """Every destination written exactly once, from the element one node up - the last node from itself."""
    for width, nodes in ((n, T + 1), (m, T)):
        count = width * nodes
        src = {}
        for e in range(count):
            for d in gs.destinations(e, width, nodes, True):
                assert d not in src, (e, d)
                src[d] = e
        assert sorted(src) == list(range(count))
        for d, e in src.items():
            assert e == (d + width if d < (nodes - 1) * width else d)
        assert all(gs.destinations(e, width, nodes, False) == [e] for e in range(count))


@pytest.mark.parametrize("complex_elems", (False, True))
@pytest.mark.parametrize("T,n,m", SHAPES)
def test_in_place_update_equals_update_then_shift(T, n, m, complex_elems):
    """In place, trip by trip: bit for bit what the update followed by shift_guess gives, and the plain update for a row that
    does not end its step.  (A trip stores at or below what it loaded, and everything below was loaded by an earlier trip.)"""
    rng = np.random.default_rng(1000 * T + 10 * n + m)
    alpha = 0.37
    for width, nodes, form in ((n, T + 1, _x_form(n, complex_elems)), (m, T, _u_form(m))):
        cx = complex_elems and width == n
        g, o = _arrays(rng, width * nodes, cx)
        got = gs.update_in_place(g.copy(), o, alpha, width, nodes, True, *form)
        want = gs.update_then_shift(g, o, alpha, width, nodes)
        assert got.tobytes() == want.tobytes()
        plain = gs.update_in_place(g.copy(), o, alpha, width, nodes, False, *form)
        assert plain.tobytes() == (g + alpha * (o - g)).tobytes()


def test_every_update_form_has_a_cell():
    forms = {(_x_form(gs.state_width(c.cell), c.cell.path == gs.kv.COMPLEX), _u_form(c.cell.nu)) for c in gs.CASES}
    assert {f[0] for f in forms} == {(2, 6), (1, 12)} and {f[1] for f in forms} == {(2, 4), (1, 8)}
    assert any(c.cell.exact for c in gs.CASES) and any(c.cell.path == gs.kv.COMPLEX for c in gs.CASES)

"""The strong-drive cases (tests/strong_drive_cases.py) on the host: the mirror of expm_cols' scaling rule against its source lines;
the preconditions that make the cases worth running (a quiet member beside one that squares three times or more, s changing along
the horizon, no norm where rounding could move s); the stored truth (tests/golden/strong_drive_truth.npz) against a recomputation
with mpmath; and the project's fp64 definitions against that truth at ONE TENTH of the bound each family's GPU test holds the
device to (1e-12 Hamiltonian / process states, 1e-11 generator states, 1e-10 max(1, max|ref|) gradients and linearisation).  The parameter
gradient runs on the same cases (sd.ParamCase): its own preconditions on the (1 + p_tot) d block of param_block_expm, its truth
(tests/golden/strong_drive_param_truth.npz) and its definition against that truth, at the end of the file."""
import importlib.util
import math
import os

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from oracle import m4q_oracle as orc
from tests import grad_cases as gc
from tests import kernel_variants as kv
from tests import plant_param_cases as pc
from tests import strong_drive_cases as sd

CASES = sd.all_cases()
IDS = [sd.case_id(*c) for c in CASES]
NOT_GEN = [c for c in CASES if not sd.is_generator(c[0])]


def rel(got, want):
    return np.abs(np.asarray(got) - np.asarray(want)).max() / max(1.0, np.abs(np.asarray(want)).max())


# ---------------------------------------------------------------- the rule and the cells
def test_squarings_mirrors_the_source_lines():
    with open(os.path.join(kv.CSRC, "m4q_mpc.h")) as fh:
        src = fh.read()
    for line in ("  const double theta13 = %r;\n" % sd.THETA13,
                 "  if (finite_d(nrm) && nrm > theta13) s = ilogb(nrm / theta13) + 1;   // NaN/inf: the result is NaN, caught upstream\n",
                 "  if (s > %d) s = %d;\n" % (sd.S_CAP, sd.S_CAP),
                 "  const double sc = ldexp(1.0, -s);\n",
                 "  for (int it = 0; __any(it < s); ++it) {\n"):
        assert src.count(line) == 1, line
    t = sd.THETA13
    assert [sd.squarings(x) for x in (0.0, 1.0, t, np.nextafter(t, 9.0), 1.99 * t, 2 * t, 2.01 * t, 4 * t, 7.9 * t, 8 * t)] \
        == [0, 0, 0, 1, 1, 2, 2, 3, 3, 4]
    for x in (5.4, 11.0, 300.0, 1e9):
        assert sd.squarings(x) == math.floor(math.log2(x / t)) + 1                   # ilogb + 1
        assert x / 2.0 ** sd.squarings(x) <= t < x / 2.0 ** (sd.squarings(x) - 1)
    assert sd.squarings(t * 2.0 ** 59.5) == 60 and sd.squarings(1e300) == 60
    assert sd.squarings(float("nan")) == 0 and sd.squarings(float("inf")) == 0


def test_the_cells_are_the_built_ones():
    sh = kv.shapes()
    names = lambda kind, fmt: sorted(fmt % nm for nm in {(nx, nu) for nx, nu, o, po in sh} if kind in kv.plant_kinds(nm[0]))
    assert names(kv.HAMILTONIAN, "%d-%d") == sorted(sd.HAMILTONIAN)
    assert names(kv.PROCESS, "%d-%d-process") == sorted(sd.PROCESS)
    assert names(kv.GENERATOR, "gen-%d-%d") == sorted(sd.GENERATOR)
    assert set(sd.QP_CELLS) < set(sd.CELLS) and set(sd.LEVEL) == set(sd.CELLS)


def test_the_generator_plant_is_the_scenarios_own():
    """gen_op0 / gen_ops as kv._finish builds them from the scenario's Hamiltonian plant."""
    p = kv.scenario(9, 2, 1)
    c = gc.plant_case("9-2")
    L0, Lk = sd._generator_ops(c, p["plant_op0"][0], p["plant_ops"][0])
    assert np.array_equal(L0, p["gen_op0"][0]) and np.array_equal(Lk, p["gen_ops"][0])


# ---------------------------------------------------------------- preconditions
@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_preconditions(key):
    cs = sd.case(*key)
    s, norms = cs.s(), cs.norms()
    assert set(s) == ({"forward"} if sd.is_generator(cs.cell) else {"forward", "block"})
    for what, a in s.items():
        print("%s %s: s =\n%s" % (cs.id, what, a))
        assert a.shape == (cs.B, cs.N)
        for b in cs.quiet:
            assert (a[b] == 0).all()                                # the quiet member never squares
        assert a[cs.driven].max() >= 3 and (cs.B == 1 or a[:4].max() >= 3)     # (in the first quad, beside the quiet one)
        if cs.N == 6:
            for b in cs.driven:
                assert len(set(a[b])) >= 2, (what, b, a[b])           # s changes along the horizon
        assert min(sd.octave_margin(x) for x in norms[what].reshape(-1)) > 1e-6
    if "block" in s:
        assert (s["block"] >= s["forward"]).all()
    # the quiet member sees controls inside the configuration's own bound
    for b in cs.quiet:
        assert np.abs(cs.v[b]).max() <= cs.c.sat
    assert np.abs(cs.v).max() > 100 * cs.c.sat


def test_the_exponents_are_the_definitions_own():
    """Case.block is grad._block_expm's matrix: its exponential holds U and dU_k where the definition reads them."""
    from scipy.linalg import expm
    from mpc4quantum_amd.grad import _block_expm
    cs = sd.case("4-2", "per", 5, 6)
    X, Es = cs.generator(0, 2)
    U, dUs = _block_expm(X, Es)
    F = expm(cs.block(0, 2))
    assert np.array_equal(F[:2, :2], U) and all(np.array_equal(F[:2, 2 + 2 * k:4 + 2 * k], dUs[k]) for k in range(2))


# ---------------------------------------------------------------- the truth
def _generator_module():
    spec = importlib.util.spec_from_file_location("make_golden_strong_drive", os.path.join(os.path.dirname(sd.TRUTH_FILE),
                                                                                            "make_golden_strong_drive.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_case_has_its_truth():
    for key in CASES:
        cs = sd.case(*key)
        tr = sd.truth(cs)
        want = {"xs", "q", "J_sum"} | (set() if sd.is_generator(cs.cell) else {"U", "dU", "grad_last", "grad_sum", "gs_last", "gs_sum"})
        assert set(tr) == want, cs.id
        assert tr["xs"].shape == (cs.B, cs.N + 1, cs.n) and all(np.isfinite(a).all() for a in tr.values())
        assert np.array_equal(tr["xs"][:, 0], cs.x0)
    assert os.path.getsize(sd.TRUTH_FILE) < 1 << 20


@pytest.mark.parametrize("cell", ["4-1", "16-1-process"])
def test_the_fixture_regenerates_bit_for_bit(cell):
    mg = _generator_module()
    for variant, B, N in sd.RUNS:
        cs = sd.case(cell, variant, B, N)
        again, stored = mg.compute(cs), sd.truth(cs)
        assert set(again) == set(stored)
        for field in stored:
            a, b = np.ascontiguousarray(again[field]), stored[field]
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (cs.id, field)


# ---------------------------------------------------------------- the definitions against the truth
@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_the_independent_chain_against_the_truth(key):
    cs = sd.case(*key)
    tr = sd.truth(cs)
    gen = sd.is_generator(cs.cell)
    step, bound = (orc.plant_step_generator, 1e-11) if gen else (cs.c.step, 1e-12)
    worst = 0.0
    for b in range(cs.B):
        op0, ops = cs.member_ops(b)
        xs = [cs.x0[b]]
        for t in range(cs.N):
            xs.append(step(xs[-1], cs.v[b, t], op0, list(ops), cs.dts[t]))
        worst = max(worst, rel(np.array(xs), tr["xs"][b]))
    print("%s: the fp64 chain against the truth %.2e (a tenth of the bound: %.1e)" % (cs.id, worst, 0.1 * bound))
    assert worst <= 0.1 * bound


@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("key", NOT_GEN, ids=[sd.case_id(*c) for c in NOT_GEN])
def test_the_gradient_definition_against_the_truth(key, figure):
    cs = sd.case(*key)
    tr = sd.truth(cs)
    ref = m4q.plant_rollout_grad_reference(cs.x0, cs.us, cs.op0, cs.ops, cs.ts, cs.W, cs.f, cs.kind, u_scale=cs.u_scale, figure=figure)
    errs = (rel(ref["q"], tr["q"][:, cs.N] if figure == "last" else tr["q"]), rel(ref["grad"], tr["grad_" + figure]),
            rel(ref["grad_scale"], tr["gs_" + figure]))
    print("%s %s: q %.2e, grad %.2e (max %.3e), grad_scale %.2e (max %.3e)"
          % (cs.id, figure, errs[0], errs[1], np.abs(tr["grad_" + figure]).max(), errs[2], np.abs(tr["gs_" + figure]).max()))
    assert max(errs) <= 1e-11
    assert np.abs(tr["grad_" + figure]).max() > 1e-3


@pytest.mark.parametrize("key", NOT_GEN, ids=[sd.case_id(*c) for c in NOT_GEN])
def test_the_linearisation_definition_against_the_truth(key):
    cs = sd.case(*key)
    tr = sd.truth(cs)
    X = np.ascontiguousarray(tr["xs"][:, :cs.N])
    ref = m4q.plant_linearize_reference(X, cs.us, cs.op0, cs.ops, cs.ts, cs.kind, u_scale=cs.u_scale)
    want = sd.linearisation(cs, tr, X)
    errs = [rel(g, w) for g, w in zip(ref, want)]
    nxt = np.einsum('btij,btj->bti', want[0], X) + np.einsum('btik,btk->bti', want[1], np.broadcast_to(cs.us, (cs.B, cs.N, cs.m))) + want[2]
    print("%s: A %.2e, B %.2e (max %.3e), Delta %.2e; A x + B u + Delta against the truth's next state %.2e"
          % (cs.id, *errs[:2], np.abs(want[1]).max(), errs[2], rel(nxt, tr["xs"][:, 1:])))
    assert max(errs) <= 1e-11
    assert rel(nxt, tr["xs"][:, 1:]) <= 1e-11 * max(1.0, np.abs(want[1]).max() * np.abs(cs.us).max())


@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("key", [c for c in NOT_GEN if c[1] == "shared" or c[2] == 1],
                         ids=[sd.case_id(*c) for c in NOT_GEN if c[1] == "shared" or c[2] == 1])
def test_the_multi_rollout_definition_against_the_truth(key, figure):
    cs = sd.case(*key)
    tr = sd.truth(cs)
    ref = m4q.plant_rollout_multi_reference(cs.x0, cs.us.reshape(cs.N, cs.m), cs.op0, cs.ops, cs.ts, cs.W, cs.f, cs.kind, u_scale=cs.u_scale,
                                            figure=figure)
    want = tr["q"][:, cs.N] if figure == "last" else tr["J_sum"]
    print("%s %s: J %.2e (max %.3e)" % (cs.id, figure, rel(ref["J"][:, 0], want), np.abs(want).max()))
    assert rel(ref["J"][:, 0], want) <= 1e-11


# ---------------------------------------------------------------- the parameter gradient
PAIRS = sd.all_param_pairs()
PAIR_IDS = [sd.pair_id(*k) for k in PAIRS]


def test_the_parameter_cells_and_sets():
    assert set(sd.PARAM_CELLS) == set(sd.QP_CELLS) and len(sd.PARAM_CELLS) == 7
    names = {pc.cell_name(nx, nu, kind) for nx, nu, kind, pt in kv.param_cells()}
    assert names == set(sd.PARAM_CELLS)                              # (16, 2) is plant-only: the C entry refuses it
    assert len(PAIRS) == 65 == len(set(PAIR_IDS)) and sd.param_sets("16-3") == [(3, False)]
    assert sd.param_sets("4-1") == [(7, False), (6, True)] and sd.param_sets("16-3-process") == [(7, False), (4, True)]
    assert set(sd.PARAM_RESEED) <= set(PAIR_IDS)


@pytest.mark.parametrize("key", PAIRS, ids=PAIR_IDS)
def test_parameter_gradient_preconditions(key):
    """The (1 + p_tot) d block of param_block_expm squares where the forward exponent does, and more.  The purpose of the sets with
    the gains in the shared layout: the quiet member's forward exponent stays at s = 0 - its u_scale is small - while its block
    squares, because the gain directions carry the UNSCALED strong control u[t][k]: s_block > s_forward inside one wavefront, the
    direction far larger than the exponent."""
    pr = sd.param_case(*key)
    cs = pr.cs
    s, norms = pr.s(), pr.norms()
    a, f = s["param_block"], s["forward"]
    print("%s: forward s =\n%s\nparam_block s =\n%s" % (pr.id, f, a))
    assert set(s) == {"forward", "param_block"} and a.shape == f.shape == (cs.B, cs.N)
    assert pr.param_block(0, 0).shape == ((1 + pr.p_tot) * cs.d,) * 2 and (1 + pr.p_tot) * cs.d <= 16
    assert a[cs.driven].max() >= 3 and (cs.B == 1 or a[:4].max() >= 3)         # (in the first quad, beside the quiet one)
    if cs.N == 6:
        for b in cs.driven:
            assert len(set(a[b])) >= 2, (b, a[b])                    # s changes along the horizon
    assert (a >= f).all()
    assert min(sd.octave_margin(x) for v in norms.values() for x in v.reshape(-1)) > 1e-6
    for b in cs.quiet:
        assert (f[b] == 0).all()
        if pr.sg and not cs.per:
            assert a[b].max() >= 1
        else:
            assert (a[b] == 0).all()
    assert np.array_equal(f, cs.s()["forward"])


def test_the_parameter_block_is_the_definitions_own():
    """ParamCase.param_block is the matrix grad._block_expm exponentiates in plant_param._param_member."""
    from scipy.linalg import expm
    from mpc4quantum_amd.grad import _block_expm
    for key in (("4-2", "shared", 5, 6, 5, True), ("9-2", "per", 5, 6, 4, False)):
        pr = sd.param_case(*key)
        d = pr.cs.d
        X, _ = pr.cs.generator(sd.QUIET, 2)
        U, dUs = _block_expm(X, pr.directions(sd.QUIET, 2))
        F = expm(pr.param_block(sd.QUIET, 2))
        assert len(dUs) == pr.p_tot and np.array_equal(F[:d, :d], U)
        assert all(np.array_equal(F[:d, (1 + e) * d:(2 + e) * d], dUs[e]) for e in range(pr.p_tot))



def _param_generator_module():
    spec = importlib.util.spec_from_file_location("make_golden_strong_drive_param", os.path.join(os.path.dirname(sd.TRUTH_FILE),
                                                                                                  "make_golden_strong_drive_param.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_pair_has_its_truth():
    for key in PAIRS:
        pr = sd.param_case(*key)
        tr = sd.param_truth(pr)
        assert set(tr) == ({"J", "grad_theta", "grad_scale"} if pr.sg else {"J", "grad_theta"}), pr.id
        assert tr["J"].shape == (pr.cs.B,) and tr["grad_theta"].shape == (pr.cs.B, pr.p) and all(np.isfinite(a).all() for a in tr.values())
        assert not pr.sg or tr["grad_scale"].shape == (pr.cs.B, pr.cs.m)
        for name in set(tr) - {"J"}:
            assert np.all(np.abs(tr[name]).max(axis=0) > 1e-3), (pr.id, name)       # no column is trivial
    assert os.path.getsize(sd.PARAM_TRUTH_FILE) < 1 << 20


# (the five runs take five times as long as the recomputation of strong_drive_truth.npz above - 1 + p_tot exponentials per member
# and step - and the two B = 5, N = 6 runs are most of it: the three short runs are recomputed, both layouts among them; the
# definition is held to every stored pair below)
REGEN_RUNS = [("shared", 5, 1), ("per", 1, 1), ("shared", 1, 6)]


@pytest.mark.parametrize("cell", ["4-1", "16-1-process"])
def test_the_parameter_fixture_regenerates_bit_for_bit(cell):
    mg = _param_generator_module()
    for variant, B, N in REGEN_RUNS:
        for p, sg in sd.param_sets(cell):
            pr = sd.param_case(cell, variant, B, N, p, sg)
            again, stored = mg.compute(pr), sd.param_truth(pr)
            assert set(again) == set(stored)
            for field in stored:
                a, b = np.ascontiguousarray(again[field]), stored[field]
                assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (pr.id, field)


@pytest.mark.parametrize("key", PAIRS, ids=PAIR_IDS)
def test_the_parameter_gradient_definition_against_the_truth(key):
    pr = sd.param_case(*key)
    tr = sd.param_truth(pr)
    args, kw = pr.args()
    ref = m4q.plant_param_grad_reference(*args, **kw)
    assert set(ref) == set(tr)
    errs = {name: rel(ref[name], tr[name]) for name in sorted(tr)}
    print("%s: %s" % (pr.id, ", ".join("%s %.2e (max %.3e)" % (name, errs[name], np.abs(tr[name]).max()) for name in sorted(tr))))
    assert max(errs.values()) <= 1e-11

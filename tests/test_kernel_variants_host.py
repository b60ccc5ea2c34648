"""CPU checks of tests/kernel_variants.py (the matrices tests/test_gpu_variant_matrix.py and tests/test_gpu_aux_matrix.py run) and of the
input shapes EnsembleSession.build_models and mpc_batch_sharded accept.

The rule lines of m4q_kernels.hip and build.py must read exactly as the Python mirrors assume: a new shape changes the matrix,
a changed rule fails here - neither can leave a compiled variant untested without notice."""
import os

import numpy as np
import pytest

from mpc4quantum_amd import configs
from mpc4quantum_amd.library import size_of_library
from mpc4quantum_amd.session import check_build_models_shapes
from oracle import m4q_oracle as orc
from tests import kernel_variants as kv


def _src(name):
    with open(os.path.join(kv.CSRC, name)) as f:
        return f.read()


# ---------------------------------------------------------------- the mirrors against the sources
def test_rule_lines_read_as_mirrored_by_path_name():
    k = _src("m4q_kernels.hip")
    for line in ("constexpr int DD = (NX == 4) ? 2 : (NX == 9) ? 3 : (NX == 16) ? 4 : 1;",
                 "constexpr bool SQUARE = DD * DD == NX;",
                 "constexpr int DQ = fourth_root(NX);",
                 "constexpr bool QUARTIC = DQ > 0;",
                 "constexpr bool HAS_TILE = SQUARE && ORDER == 1 && NX - 1 <= 8;",
                 "constexpr bool HAS_SG = SQUARE && ORDER == 1 && NX == 16;"):
        assert k.count(line) == 1, line
    # pick_kernel: !SQUARE runs PLANT_NONE on PATH_COMPLEX alone; PATH_SG only unexact where HAS_SG; PATH_TILE only unexact where
    # HAS_TILE; everything else on the traceless coordinates (coords_of: PATH_TRACELESS, PATH_TILE, PATH_SG) runs the traceless kernel
    body = k[k.index("static int pick_kernel("):k.index("#ifndef M4Q_PLANT_ONLY\nstatic int launch_mpc")]
    assert "if (path != PATH_COMPLEX || plant_kind != PLANT_NONE) return unsupported;" in body
    assert "if (path == PATH_SG && !exact) return pick_plant<double, false, true, false, Op, true>(op, plant_kind);" in body
    assert "if (path == PATH_SG) path = PATH_TRACELESS;" in body
    assert ("if constexpr (HAS_TILE) { if (path == PATH_TILE && !exact) return pick_plant<double, false, true, true>(op, plant_kind); }"
            in body)
    assert ("if (coords_of(path) == COORDS_TRACELESS) return exact ? pick_plant<double, true, true, false>(op, plant_kind) : "
            "pick_plant<double, false, true, false>(op, plant_kind);") in body
    assert _src("m4q_args.h").count("constexpr Coords coords_of(Path p) { return p == PATH_COMPLEX ? COORDS_COMPLEX : "
                                    "p == PATH_REAL ? COORDS_HERM : COORDS_TRACELESS; }") == 1
    assert ("if (path == PATH_REAL) return exact ? pick_plant<double, true, false, false>(op, plant_kind) : "
            "pick_plant<double, false, false, false>(op, plant_kind);") in body
    assert ("return exact ? pick_plant<cplx, true, false, false>(op, plant_kind) : pick_plant<cplx, false, false, false>(op, "
            "plant_kind);") in body
    # pick_plant: the generator plant in the gen object alone, the process plant on quartic complex kernels alone
    body = k[k.index("static int pick_plant("):k.index("static int pick_kernel(")]
    assert body.count("return op.template run<S, PLANT_NONE, EXACT, false, false>();") == 1          # !SQUARE
    assert "if (plant_kind == PLANT_GENERATOR) return op.template run<S, PLANT_GENERATOR, EXACT, TL, TILE, SG>();" in body
    assert "if (plant_kind == PLANT_HAMILTONIAN) return op.template run<S, PLANT_HAMILTONIAN, EXACT, TL, TILE, SG>();" in body
    assert ("if constexpr (QUARTIC && std::is_same<S, cplx>::value && !TL && !TILE && !SG) return op.template run<S, PLANT_PROCESS, "
            "EXACT, false, false>();") in body
    assert "return op.template run<S, PLANT_NONE, EXACT, TL, TILE, SG>();" in body
    b = _src("build.py")
    assert b.count("d = {4: 2, 9: 3, 16: 4}.get(nx)") == 1 and b.count("if d and not plant_only:") == 1
    assert '"-DM4Q_VARIANT_GEN"' in b


def test_piece_rule_lines_read_as_mirrored():
    """The cut rule kernel_variants.pieces() mirrors (mpc_kernel: XCUTS, two_phase, the exact kernel's n_pieces loop, piece_cut and
    the item's [row_begin, row_end)), by exact text."""
    k = _src("m4q_kernels.hip")
    for text in ("constexpr int XCUTS[] = {4, 7, 12};",
                 "    two_phase = a->step_begin < 2 && a->step_end > 2;\n",
                 "    n_pieces = two_phase ? 2 : 1;\n"
                 "    if constexpr (EXACT) {\n"
                 "#pragma unroll\n"
                 "      for (int i = 0; i < NXC; ++i)\n"
                 "        if (two_phase && a->step_end > XCUTS[i]) ++n_pieces;\n"
                 "    }\n",
                 "    int v = 2;\n"
                 "#pragma unroll\n"
                 "    for (int k = 0; k < NXC; ++k)\n"
                 "      if (i == k + 2) v = XCUTS[k];\n"
                 "    return v;\n",
                 "          row_begin = ph == 0 ? step_begin : piece_cut(ph);\n"
                 "          row_end = ph == n_pieces - 1 ? step_end : piece_cut(ph + 1);\n"):
        assert k.count(text) == 1, text


def test_constant_target_rule_lines_read_as_mirrored():
    """kernel_variants.TC_MIN_N / has_tc against the lines of mpc_kernel they mirror, the exact kernel's pin.tconst, and the two
    host-side lines the moving-target cases of tests/operand_cases.py rest on: the tile path needs a constant target, and the flag
    is the session's targ_const."""
    k, capi = _src("m4q_kernels.hip"), _src("m4q_capi.hip")
    assert k.count("constexpr int TC_MIN_N = %d;" % kv.TC_MIN_N) == 1
    assert k.count("        constexpr bool HAS_TC = NS >= TC_MIN_N && sizeof(S) == sizeof(double);\n") == 1
    assert k.count("        if constexpr (HAS_TC) tc = (flags & QP_TARG_CONST) != 0;\n") == 1
    assert k.count("        pin.tconst = (flags & QP_TARG_CONST) != 0;\n") == 1
    assert capi.count("    const bool supported[m4q::PATH_SG + 1] = {true, real, traceless, traceless && targ_const, traceless && sg_ok};") == 1
    assert capi.count("  a.flags = p.qp_flags | (s->targ_const ? m4q::QP_TARG_CONST : 0) | ") == 1
    cases = ((4, kv.REAL), (9, kv.REAL), (9, kv.TRACELESS), (9, kv.TILE), (16, kv.SG), (16, kv.COMPLEX), (8, kv.COMPLEX))
    assert [kv.has_tc(nx, path) for nx, path in cases] == [False, True, True, False, True, False, False]
    assert kv.n_state(9, kv.TRACELESS) == 8 and kv.n_state(9, kv.REAL) == 9 and kv.n_state(4, kv.TILE) == 3


def test_pieces_mirror_the_cut_rule():
    assert kv.XCUTS == (4, 7, 12) and kv.LONG_STEPS > kv.XCUTS[-1] + 1
    assert kv.pieces(0, 14, True) == [(0, 2), (2, 4), (4, 7), (7, 12), (12, 14)]
    assert kv.pieces(0, 14, False) == [(0, 2), (2, 14)]
    assert kv.pieces(1, 5, True) == [(1, 2), (2, 4), (4, 5)]
    assert kv.pieces(0, 4, True) == [(0, 2), (2, 4)]
    assert kv.pieces(3, 14, True) == [(3, 14)]
    for exact in (False, True):
        assert kv.pieces(0, 2, exact) == [(0, 2)]
        # every launch range is tiled by non-empty pieces
        for b in range(kv.LONG_STEPS):
            for e in range(b + 1, kv.LONG_STEPS + 1):
                ps = kv.pieces(b, e, exact)
                assert ps[0][0] == b and ps[-1][1] == e and all(lo < hi for lo, hi in ps), (b, e, ps)
                assert all(p[1] == q[0] for p, q in zip(ps, ps[1:])), (b, e, ps)


def test_mirrors_agree_with_the_rule_text():
    for nx in (4, 8, 9, 16):
        assert kv.square(nx) == (nx in (4, 9, 16)) and kv.quartic(nx) == (nx == 16)
    assert [kv.fourth_root(n) for n in (1, 4, 8, 9, 16, 81)] == [1, 0, 0, 0, 2, 3]
    assert kv.has_tile(4, 1) and kv.has_tile(9, 1) and not kv.has_tile(16, 1) and not kv.has_tile(4, 2)
    assert kv.has_sg(16, 1) and not kv.has_sg(16, 2) and not kv.has_sg(9, 1)


# ---------------------------------------------------------------- the matrix
def test_spot_check_of_the_cells():
    cells = kv.closed_loop_cells()
    ids = [kv.cell_id(c) for c in cells]
    assert len(ids) == len(set(ids))
    shape = {}
    for c in cells:
        shape.setdefault((c.nx, c.nu, c.order), []).append(c)
    # (8, 2, 1): the complex kernel with no plant, clipped and exact - nothing else is built
    assert sorted((c.path, c.exact, c.plant) for c in shape[(8, 2, 1)]) == [(kv.COMPLEX, False, kv.NONE), (kv.COMPLEX, True, kv.NONE)]
    # (16, 2, 1) is plant-only: no closed-loop cell, plant cells only
    assert (16, 2, 1) not in shape
    entry = kv.entry_point_cells()
    assert [(c.kind, c.mode) for c in entry if (c.nx, c.nu) == (16, 2)] == [("plant", kv.HAMILTONIAN), ("plant", kv.GENERATOR)]
    # the shared-generator kernel at (16, 1, 1), clipped only, under each plant it is built with; none at (16, 1, 2)
    sg = [c for c in shape[(16, 1, 1)] if c.path == kv.SG]
    assert sorted(c.plant for c in sg) == sorted([kv.NONE, kv.HAMILTONIAN, kv.GENERATOR]) and not any(c.exact for c in sg)
    assert not any(c.path == kv.SG for c in shape[(16, 1, 2)])
    # the process plant: complex path, quartic shapes, both solves
    proc = sorted((c.nx, c.nu, c.order, c.path, c.exact) for c in cells if c.plant == kv.PROCESS)
    assert proc == sorted((16, nu, o, kv.COMPLEX, e) for nu, o in ((1, 1), (1, 2), (1, 3), (1, 4), (3, 1)) for e in (False, True))
    # tile cells (clipped backward sweep, exact pinned sweep) exactly where HAS_TILE
    assert sorted({(c.nx, c.order) for c in cells if c.path == kv.TILE}) == [(4, 1), (9, 1)]
    assert all(c.plant != kv.GENERATOR or kv.square(c.nx) for c in cells)
    # per shape: (clipped paths + exact paths) x (none, hamiltonian, generator) + the process cells
    for (nx, nu, o), cs in shape.items():
        n_paths = len(kv.clipped_paths(nx, o)) + len(kv.exact_paths(nx, o))
        expect = n_paths * (3 if kv.square(nx) else 1) + (2 if kv.quartic(nx) else 0)
        assert len(cs) == expect, (nx, nu, o)
    qp = {(c.nx, c.nu) for c in entry if c.kind == "qp"}
    assert qp == {(4, 1), (4, 2), (9, 2), (16, 3), (16, 1), (8, 2)}
    assert {(c.nx, c.nu, c.order) for c in entry if c.kind == "discretize"} == {
        (4, 1, 1), (4, 1, 2), (4, 2, 1), (9, 2, 1), (9, 2, 2), (16, 3, 1), (16, 1, 1), (16, 1, 2), (8, 2, 1)}


# ---------------------------------------------------------------- the auxiliary families
def test_aux_rule_lines_read_as_mirrored():
    """What kernel_variants.aux_cells() mirrors, by exact text: which objects hold the auxiliary kernels at all, the two layouts
    that decide where the fit and online kernels are built, the plant dispatch, the refusals and the grid cap."""
    k, b, capi = _src("m4q_kernels.hip"), _src("build.py"), _src("m4q_capi.hip")
    fit_h, online_h = _src("m4q_fit.h"), _src("m4q_online.h")
    # plant-only shapes and the gen object hold no auxiliary kernel but the plant families
    assert k.count("#if defined(M4Q_PLANT_ONLY) || defined(M4Q_VARIANT_GEN)\n#define M4Q_NO_AUX 1\n") == 1
    assert b.count('(["-DM4Q_PLANT_ONLY"] if plant_only else [])') == 1
    assert b.count('return [(int(a), int(b), int(c), "plant-only" in rest)') == 1
    assert k.count("#ifndef M4Q_NO_AUX\nstatic int launch_model_grad(const GradArgs& a, hipStream_t s) {\n  const int rc = launch_rows("
                   "model_rollout_grad_kernel, a, a.roll.B, MODEL_LDS, s);\n") == 1
    for line in ("static int launch_model_rollout(const RollArgs& a, hipStream_t s) { return launch_aux(model_rollout_kernel, a, MODEL_LDS, s); }",
                 "static int launch_model_feedback(const FeedbackArgs& a, hipStream_t s) { return launch_rows(model_feedback_kernel, a, "
                 "a.roll.B, MODEL_LDS, s); }"):
        assert k.count(line) == 1, line
    # FitLayout / OnlineLayout
    assert fit_h.count("constexpr size_t FIT_LDS_LIMIT = 160 * 1024;") == 1
    for text, line, n in ((fit_h, "  static constexpr int NZ = NX * (1 + PowTab<NU, ORDER>::NP);", 1),
                          (fit_h, "  static constexpr int PITCH = NZ | 1;", 1),
                          (fit_h, "  static constexpr int G = 0, V = G + NZ * PITCH, C = V + NZ * PITCH, Z = C + NX * PITCH, XN = Z + NZ, "
                                  "LAM = XN + NX;", 1),
                          (fit_h, "  static constexpr int ELEMS = LAM + (NZ + 1) / 2;", 1),
                          (fit_h, "  static constexpr size_t BYTES = sizeof(cplx) * (size_t)ELEMS;", 1),
                          (fit_h, "  static constexpr bool FITS = NZ <= 64 && BYTES <= FIT_LDS_LIMIT;", 1),
                          (online_h, "  static constexpr int NZ = NX * (1 + PowTab<NU, ORDER>::NP);", 1),
                          (online_h, "  static constexpr int PITCH = NZ | 1;", 1),
                          (online_h, "  static constexpr int P = 0, A = P + NZ * PITCH, Z = A + NX * PITCH, XN = Z + NZ, PZ = XN + NX, "
                                     "W = PZ + NZ, R = W + NZ, GR = R + NX;", 1),
                          (online_h, "  static constexpr int ELEMS = GR + NX;", 1),
                          (online_h, "  static constexpr size_t BYTES = sizeof(cplx) * (size_t)ELEMS;", 1),
                          (online_h, "  static constexpr bool FITS = NZ <= 64 && BYTES <= FIT_LDS_LIMIT;", 1)):
        assert text.count(line) == n, line
    for line in ("constexpr bool FIT_FITS = FitLayout<NX, NU, ORDER>::FITS;",
                 "constexpr int FIT_LDS = FIT_FITS ? (int)FitLayout<NX, NU, ORDER>::BYTES : 0;",
                 "constexpr bool ONLINE_FITS = OnlineLayout<NX, NU, ORDER>::FITS;",
                 "constexpr int ONLINE_LDS = ONLINE_FITS ? (int)OnlineLayout<NX, NU, ORDER>::BYTES : 0;",
                 "  static int run(const OnlineArgs& a, int hermitian, hipStream_t s) { return hermitian ? go<true>(a, s) : go<false>(a, s); }"):
        assert k.count(line) == 1, line
    assert capi.count("  if (sh->fit_lds_bytes == 0)\n    return fail(M4Q_E_UNSUPPORTED, ") == 1
    assert capi.count("  if (sh->online_lds_bytes == 0)\n    return fail(M4Q_E_UNSUPPORTED, ") == 1
    # the plant dispatch, written once: launch_by_plant<GEN>, GEN for the families with a generator-plant kernel
    body = k[k.index("static int launch_by_plant("):k.index("static int launch_plant(const PlantArgs& a")]
    for line in ("  if constexpr (!SQUARE) {\n    return UNBUILT;\n",
                 "    const auto go = [&](auto plant) { return launch_rows(kernel_of(plant), a, count, sizeof(cplx) * (size_t)(ROWS * "
                 "lds_elems(plant)), s); };\n",
                 "    if (kind == PLANT_HAMILTONIAN) return go(ic<PLANT_HAMILTONIAN>{});\n",
                 "    if (kind == PLANT_PROCESS) {\n      if constexpr (QUARTIC) return go(ic<PLANT_PROCESS>{});\n"
                 "      else return UNBUILT;\n    }\n",
                 "    if constexpr (GEN) return go(ic<PLANT_GENERATOR>{});\n    else return UNBUILT;\n"):
        assert body.count(line) == 1, line
    # plant_kernel, plant_rollout_kernel and plant_feedback_kernel: all three plants
    for line in ("  return launch_by_plant<true>(a, a.kind, a.B, s, [](auto plant) { return plant_kernel<decltype(plant)::value>; }, step_lds);\n",
                 "  return launch_by_plant<true>(a, a.kind, a.B, s, [](auto plant) { return plant_rollout_kernel<decltype(plant)::value>; }, "
                 "step_lds);\n",
                 "  return launch_by_plant<true>(a, a.roll.kind, a.roll.B, s, [](auto plant) { return plant_feedback_kernel<decltype(plant)::"
                 "value>; }, step_lds);\n"):
        assert k.count(line) == 1, line
    assert k.count("launch_by_plant<true>(") == 3
    # the gradient and the linearisation: Hamiltonian, process where QUARTIC, nothing else - and the entry points refuse the generator
    body = k[k.index("static int launch_plant_grad("):k.index("// a linearisation kernel over quads")]
    assert body.count("  const int rc = launch_by_plant<false>(a, a.roll.kind, a.roll.B, s, [](auto plant) { return plant_rollout_grad_kernel<"
                      "decltype(plant)::value>; },\n") == 1
    assert body.count("launch_by_plant<") == 1 and "PLANT_GENERATOR" not in body
    body = k[k.index("static int launch_plant_linearize("):k.index("#ifndef M4Q_NO_AUX\nstatic int launch_model_grad(")]
    assert body.count("  return launch_by_plant<false>(a, a.kind, a.B * a.T, s, [](auto plant) { return plant_linearize_kernel<"
                      "decltype(plant)::value>; }, lin_lds);\n") == 1
    assert body.count("launch_by_plant<") == 1 and "PLANT_GENERATOR" not in body
    assert capi.count('  if (lacks && kind == M4Q_PLANT_GENERATOR)\n    return fail(M4Q_E_UNSUPPORTED, "%s: the generator plant has no %s '
                      '(its block matrix has (1 + m) n > 16 columns): %s", who, lacks, advice);\n') == 1
    assert capi.count('  if (int rc = check_plant_kind(who, /*named=*/false, plant_kind, dim_x, "gradient kernel",\n') == 1
    assert capi.count('  if (int rc = check_plant_kind(who, /*named=*/false, plant_kind, dim_x, "linearisation kernel",\n') == 1
    assert capi.count("  if (int rc = check_plant_kind(who, /*named=*/false, plant_kind, dim_x, nullptr, nullptr)) return rc;\n") == 2
    # one object per (n, m) serves every plant family, plant-only shapes included; the model families need the shape's own object
    assert capi.count("  const m4q::ShapeOps* sh = find_shape_any_order(dim_x, dim_u, /*plant_ok=*/true);") == 1      # m4q_plant_step_batch
    assert capi.count("  *found = find_shape_any_order(dim_x, dim_u, /*plant_ok=*/true);") == 1                        # plant_shape
    assert capi.count("  if (int rc = plant_shape(who, /*named=*/false, dim_x, dim_u, /*needs_qp=*/false, &sh)) return rc;") == 4
    assert capi.count("    if (s->nx == nx && s->nu == nu && s->order == order && (plant_ok || !s->plant_only)) return s;") == 1
    # the grid cap of every auxiliary launch
    assert k.count("constexpr int ROWS = 4;") == 1
    assert k.count("  const int nquads = (B + ROWS - 1) / ROWS;\n  return nquads < 4096 ? (nquads > 0 ? nquads : 1) : 4096;\n") == 1
    assert k.count("  hipLaunchKernelGGL(kern, dim3(B < 4096 ? B : 4096), dim3(64), lds, s, a);") == 1   # launch_members
    assert k.count(", a, a.B, LDS, s); }") == 2 and k.count(", a, a.B, OnlineLayout<N_, NU, ORDER>::BYTES, s);") == 1   # fit, fit_qr, online
    assert k.count(", a, a.fit.B, LDS, s); }") == 2                                                       # refit, refit_qr
    assert k.count("launch_members(") == 6
    assert k.count("  hipLaunchKernelGGL(kern, dim3(grid_for(count)), dim3(64), lds, s, a);") == 1       # launch_rows
    assert k.count("{ return launch_rows(kern, a, a.B, lds, s); }") == 1                                  # launch_aux
    assert k.count("hipLaunchKernelGGL(") == 8     # mpc_kernel; launch_rows, launch_members; noise; the two reductions' two passes
    assert (kv.AUX_GRID, kv.ROWS, kv.QUAD_WRAP, kv.FIT_LDS_LIMIT) == (4096, 4, 16384, 160 * 1024)


def test_aux_mirrors_agree_with_the_rule_text():
    for nu, order in ((1, 1), (2, 1), (3, 1), (1, 2), (2, 2), (1, 3), (1, 4)):
        assert kv.n_lifted(nu, order) == size_of_library(order, nu) - 1
    assert [kv.lifted_size(*s[:3]) for s in kv.shapes()] == [8, 12, 12, 27, 54, 64, 32, 48, 64, 80, 24, 48]
    # FitLayout at (16, 3, 1), the largest that fits: 2 * 64 * 65 + 16 * 65 + 64 + 16 + 32 complex entries
    assert kv.fit_lds_bytes(16, 3, 1) == 16 * 9472 and kv.fit_lds_bytes(16, 3, 1) <= kv.FIT_LDS_LIMIT < kv.fit_lds_bytes(16, 1, 4)
    assert kv.online_lds_bytes(4, 1, 1) == 16 * (8 * 9 + 4 * 9 + 8 + 4 + 8 + 8 + 4 + 4)
    assert kv.fit_fits(16, 3, 1) and kv.online_fits(16, 1, 3) and not kv.fit_fits(16, 1, 4) and not kv.online_fits(16, 1, 4)
    assert kv.plant_kinds(8) == [] and kv.plant_kinds(9) == [kv.HAMILTONIAN, kv.GENERATOR]
    assert kv.plant_kinds(16) == [kv.HAMILTONIAN, kv.GENERATOR, kv.PROCESS]


def test_spot_check_of_the_aux_cells():
    cells = kv.aux_cells()
    ids = [kv.aux_cell_id(c) for c in cells]
    assert len(ids) == len(set(ids))
    by = {}
    for c in cells:
        by.setdefault(c.family, []).append(c)
    assert set(by) == set(kv.MODEL_FAMILIES) | set(kv.FIT_FAMILIES) | set(kv.PLANT_FAMILIES) | {"online"}
    model_shapes = [(4, 1, 1), (4, 1, 2), (4, 2, 1), (9, 2, 1), (9, 2, 2), (16, 3, 1), (16, 1, 1), (16, 1, 2), (16, 1, 3), (16, 1, 4), (8, 2, 1)]
    fitting = [s for s in model_shapes if s != (16, 1, 4)]
    for f in kv.MODEL_FAMILIES:                                    # the eleven objects with the model kernels, (16, 1, 4) among them
        assert [(c.nx, c.nu, c.order, c.kind) for c in by[f]] == [s + ("-",) for s in model_shapes]
    for f in kv.FIT_FAMILIES:                                      # the ten fitting shapes; (16, 1, 4), nz = 80, refused
        assert [(c.nx, c.nu, c.order) for c in by[f] if c.kind == "-"] == fitting
        assert [(c.nx, c.nu, c.order) for c in by[f] if c.kind == kv.REFUSED] == [(16, 1, 4)] and len(by[f]) == 11
    for form in (kv.PLAIN, kv.HERMITIAN_FORM):
        assert [(c.nx, c.nu, c.order) for c in by["online"] if c.kind == form] == fitting
    assert [(c.nx, c.nu, c.order) for c in by["online"] if c.kind == kv.REFUSED] == [(16, 1, 4)] and len(by["online"]) == 21
    # (16, 2): the plant families alone
    assert {c.family for c in cells if (c.nx, c.nu) == (16, 2)} == set(kv.PLANT_FAMILIES)
    assert not any(c.nx == 8 for f in kv.PLANT_FAMILIES for c in by[f])
    nm = [(4, 1), (4, 2), (9, 2), (16, 1), (16, 2), (16, 3)]
    for f in ("plant_rollout", "plant_feedback"):
        for kind in (kv.HAMILTONIAN, kv.GENERATOR):
            assert [(c.nx, c.nu) for c in by[f] if c.kind == kind] == nm
        assert not any(c.kind == kv.REFUSED for c in by[f])
    for f in ("plant_grad", "plant_linearize"):
        assert [(c.nx, c.nu) for c in by[f] if c.kind == kv.HAMILTONIAN] == nm
        assert [(c.nx, c.nu) for c in by[f] if c.kind == kv.REFUSED] == nm and not any(c.kind == kv.GENERATOR for c in by[f])
    for f in kv.PLANT_FAMILIES:                                    # the process cells: the quartic (n, m)
        assert [(c.nx, c.nu) for c in by[f] if c.kind == kv.PROCESS] == [(16, 1), (16, 2), (16, 3)]
        assert all(c.order == 0 for c in by[f])
    assert len(cells) == 3 * 11 + 4 * 11 + 21 + 4 * (2 * 6 + 3)


def test_a_dropped_shape_changes_the_aux_cells(monkeypatch, tmp_path):
    """aux_cells() on a copy of build.py and m4q_shapes.inc with one shape line deleted loses that shape's cells and no other (the
    rule lines themselves are pinned above: an edited one fails there)."""
    import shutil
    full = kv.aux_cells()
    for name in ("build.py", "m4q_shapes.inc"):
        shutil.copy(os.path.join(kv.CSRC, name), tmp_path / name)
    inc = tmp_path / "m4q_shapes.inc"
    assert inc.read_text().count("M4Q_SHAPE(16, 1, 3)\n") == 1
    inc.write_text(inc.read_text().replace("M4Q_SHAPE(16, 1, 3)\n", ""))
    monkeypatch.setattr(kv, "CSRC", str(tmp_path))
    fewer = kv.aux_cells()
    assert set(full) - set(fewer) == {c for c in full if (c.nx, c.nu, c.order) == (16, 1, 3)} and set(fewer) <= set(full)
    assert len(full) - len(fewer) == 3 + 4 + 2


def test_every_closed_loop_shape_has_a_scenario():
    for nx, nu, order, plant_only in kv.shapes():
        if plant_only:
            with pytest.raises(KeyError):
                kv.scenario(nx, nu, order)
        else:
            assert kv.scenario(nx, nu, order)["dim_x"] == nx


def _density(x, d):
    rho = np.reshape(x, (d, d))
    return np.abs(rho - rho.conj().T).max() <= 1e-14 and abs(np.trace(rho) - 1) <= 1e-14


@pytest.mark.parametrize("shape", [s[:3] for s in kv.shapes() if not s[3]], ids=lambda s: "%d-%d-%d" % s)
def test_scenario_is_well_formed(shape):
    """States and targets Hermitian with unit trace (two of them side by side at n = 8); models equal the oracle's expansion of the
    scaled generators; every operator has the shape the C ABI reads; bounds and sizes as the matrix wants them."""
    nx, nu, order = shape
    p = kv.scenario(nx, nu, order)
    B, n, m, T, ns = p["batch"], p["dim_x"], p["dim_u"], p["horizon"], p["n_steps"]
    assert (B, T, ns) == (kv.BATCH, kv.HORIZON, kv.STEPS) and T % 4 != 0 and T > 4
    P = size_of_library(order, m) - 1
    assert p["models"].shape == (B, n, n * (1 + P)) and p["generators"].shape == (1 + m, n, n) and p["scales"].shape == (B, 1 + m)
    assert p["x0"].shape == (B, n) and p["X_targ"].shape == (n, ns + T + 1) and p["U_targ"].shape == (m, ns + T)
    assert p["Q"].shape == p["Qf"].shape == (n, n) and p["R"].shape == (m, m) and p["sat"] > 0
    parts = [(slice(0, 4), 2), (slice(4, 8), 2)] if n == 8 else [(slice(0, n), kv.dd(n))]
    for sl, d in parts:
        assert all(_density(x[sl], d) for x in p["x0"])
        assert all(_density(x[sl], d) for x in p["X_targ"].T)
    assert len({tuple(np.round(x, 12)) for x in p["x0"]}) == B                      # distinct members
    for b in range(B):
        ref = orc.discretize_homogeneous([p["scales"][b, k] * p["generators"][k] for k in range(1 + m)], p["dt"], order)
        assert np.abs(p["models"][b] - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    assert np.abs(p["models"][0] - p["models"][1]).max() > 1e-6
    if kv.square(n):
        d = kv.dd(n)
        assert p["plant_op0"].shape == (1, d, d) and p["plant_ops"].shape == (1, m, d, d)
        assert p["gen_op0"].shape == (1, n, n) and p["gen_ops"].shape == (1, m, n, n)
        # the generator plant is trace preserving (so the traceless path applies) and dissipative (not a Liouvillian)
        eye = np.eye(d).reshape(-1)
        assert np.abs(eye @ p["gen_op0"][0]).max() <= 1e-14 and np.abs(p["gen_op0"][0] @ eye).max() > 1e-3
    else:
        assert p["gen_op0"].shape == (1, n, n) and p["gen_ops"].shape == (1, m, n, n)


@pytest.mark.parametrize("nu,order", sorted({(c.nu, c.order) for c in kv.closed_loop_cells() if c.plant == kv.PROCESS}))
def test_process_scenario_is_well_formed(nu, order):
    p = kv.process_scenario(nu, order)
    B, m = p["batch"], p["dim_u"]
    P = size_of_library(order, m) - 1
    assert m == nu and p["models"].shape == (1, 16, 16 * (1 + P)) and p["U_targ"].shape[0] == m and p["R"].shape == (m, m)
    assert p["x0"].shape == (B, 16) and p["plant_op0"].shape == (B, 2, 2) and p["plant_ops"].shape == (1, m, 2, 2)
    assert p["gen_op0"].shape == (B, 16, 16) and p["gen_ops"].shape == (1, m, 16, 16)
    ref = orc.discretize_homogeneous(list(p["generators"]), p["dt"], order)
    assert np.abs(p["models"][0] - ref).max() <= 1e-13
    for x in p["x0"]:
        M = x.reshape(4, 4)
        assert np.abs(M @ M.conj().T - np.eye(4)).max() <= 1e-14            # U (x) U^* is unitary
    assert len({round(float(h[0, 0].real), 12) for h in p["plant_op0"]}) == B   # detuned members
    assert np.abs(p["U_targ"]).max() > p["sat"]                              # the reference ramps past the bound


# ---------------------------------------------------------------- build_models / mpc_batch_sharded input shapes
def test_build_models_shape_check():
    B, n, m = 5, 16, 3
    g = np.zeros((1 + m, n, n))
    sc = np.ones((B, 1 + m))
    for gens in (g, g[None], np.stack([g] * B)):
        for scales in (None, sc):
            check_build_models_shapes(B, n, m, gens, scales)
    bad = [(g, sc[0]), (g, sc[:, 0]), (g, sc[:-1]), (g, np.ones((B, m))), (g, sc[None]),       # scales
           (np.stack([g] * (B - 1)), None), (np.stack([g] * 2), sc), (g[:-1], None), (g[None, None], None),
           (np.zeros((1 + m, n, n - 1)), None), (np.zeros((1 + m, 9, 9)), None)]                  # generators
    for gens, scales in bad:
        with pytest.raises(ValueError):
            check_build_models_shapes(B, n, m, gens, scales)


class _Rank1Of2:
    """A host transport as rank 1 of two: its block is [3, 5) of five members, the gather goes to rank 0 (None here)."""
    on_device = False
    rank, world = 1, 2

    def gather_host(self, buf, dst):
        return None

    def wait(self, slot=-1):
        pass


def _sharded(**kw):
    import mpc4quantum_amd as m4q
    from mpc4quantum_amd.distributed import mpc_batch_sharded
    p = configs.build(4, batch=5, horizon=4, n_steps=2)
    seen = {}

    def solver(x0, models, dim_u, order, X_targ, U_targ, clock, op0, ops, Q, R, Qf, sat, du, **skw):
        seen.update(skw, x0=x0)
        b = len(x0)
        return {"xs": np.zeros((b, 16, 3), complex), "us": np.zeros((b, 3, 2)), "exit_codes": np.zeros(b, np.int32),
                "steps_done": np.full(b, 2, np.int32), "qp_solves": np.ones((b, 2), np.int32)}
    args = dict(generators=p["generators"], scales=p["scales"])
    args.update(kw)
    models = args.pop("models", None)
    out = mpc_batch_sharded(p["x0"], models, 3, 1, p["X_targ"], p["U_targ"], m4q.StepClock(p["dt"], 4, 2), p["plant_op0"],
                            p["plant_ops"], p["Q"], p["R"], p["Qf"], p["sat"], p["du"], transport=_Rank1Of2(), solver=solver, **args)
    return p, out, seen


def test_sharded_scales_are_sliced_by_member():
    p, out, seen = _sharded()
    assert out is None                                                       # not the gathering rank
    assert np.array_equal(seen["scales"], p["scales"][3:5]) and np.array_equal(seen["x0"], p["x0"][3:5])
    assert np.array_equal(seen["generators"], p["generators"])               # one shared set: every rank gets it whole
    per = np.stack([p["generators"] * (1 + 0.1 * b) for b in range(5)])
    _, _, seen = _sharded(generators=per)
    assert np.array_equal(seen["generators"], per[3:5])


def test_sharded_rejects_bad_scales_and_models_with_generators():
    p = configs.build(4, batch=5, horizon=4, n_steps=2)
    for scales in (p["scales"][0], p["scales"][:, 0], p["scales"][:4], p["scales"].T):
        with pytest.raises(ValueError, match="scales"):
            _sharded(scales=scales)
    with pytest.raises(ValueError, match="not both"):
        _sharded(models=np.zeros((1, 16, 64), complex))

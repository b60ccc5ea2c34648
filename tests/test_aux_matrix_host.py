"""CPU checks of tests/aux_matrix_cases.py: the definitions alone, evaluated on the inputs of every cell of
kernel_variants.aux_cells(), meet the preconditions the comparisons of tests/test_gpu_aux_matrix.py rest on - so that a weak case
fails here and not silently on the device.

  model / plant rollout   the reference chain is finite, the members differ and move, the random controls are of the bound's size
  gradients               max |grad_ref| > 1e-3 (tests/test_gpu_grad.py)
  plant linearisation     max |B_ref| > 1e-3 (tests/test_gpu_plant_linearize.py)
  feedback                the definition's own run reaches the lower bound, the upper bound, the interior and the band (fc.activity)
  fit families            what synthetic() enforces - every cut-off a factor 1.2 clear of every singular value of every member, one
                          that truncates - and one cut-off per cell whose Gram bound is at most 1e-8
  online                  the definition moves by s <= 1e-11 under a 1e-15 perturbation of the data (tests/test_gpu_online.py)
  refused                 the cell is refused by the rule it is listed under"""
import numpy as np
import pytest

from mpc4quantum_amd import fit
from tests import aux_matrix_cases as amc
from tests import kernel_variants as kv
from tests.test_fit_host import model_bounds as gram_bounds
from tests.test_fit_qr_host import model_bounds as qr_bounds
from tests.test_gpu_online import sensitivity

CELLS = kv.aux_cells()


def _cells(*families):
    return [c for c in CELLS if c.family in families]


def test_every_cell_has_a_builder():
    assert {c.family for c in CELLS} == set(kv.MODEL_FAMILIES) | set(kv.FIT_FAMILIES) | set(kv.PLANT_FAMILIES) | {"online"}
    assert amc.B == 5 and amc.N_ROLL == 7 and amc.N_GRAD == 6 and amc.N_FEEDBACK == 8


@pytest.mark.parametrize("cell", [c for c in CELLS if c.kind == kv.REFUSED], ids=kv.aux_cell_id)
def test_refused_cells_are_refused_by_rule(cell):
    if cell.family in kv.PLANT_FAMILIES:
        assert cell.family in ("plant_grad", "plant_linearize") and kv.GENERATOR in kv.plant_kinds(cell.nx)
    else:
        assert kv.lifted_size(cell.nx, cell.nu, cell.order) > 64


@pytest.mark.parametrize("variant", amc.VARIANTS)
@pytest.mark.parametrize("cell", _cells("model_rollout", "plant_rollout"), ids=kv.aux_cell_id)
def test_rollout_inputs(cell, variant):
    if cell.family == "model_rollout":
        c = amc.model_rollout_case(cell.nx, cell.nu, cell.order, variant)
        ref, sat = amc.model_rollout_reference(c), c["sat"]
    else:
        c = amc.plant_rollout_case(cell.nx, cell.nu, cell.kind, variant)
        ref, sat = amc.plant_rollout_reference(c), c["c"].sat
    assert ref.shape == (amc.B, amc.N_ROLL + 1, cell.nx) and np.isfinite(ref).all()
    assert 0.1 * sat < np.abs(c["u"]).max() <= sat
    assert len({np.round(x, 9).tobytes() for x in ref[:, -1]}) == amc.B                   # the members do differ
    assert np.abs(ref[:, -1] - ref[:, 0]).max() > 1e-3                                    # ... and move


@pytest.mark.parametrize("variant", amc.VARIANTS)
@pytest.mark.parametrize("cell", [c for c in _cells("model_grad", "plant_grad") if c.kind != kv.REFUSED], ids=kv.aux_cell_id)
def test_gradient_inputs(cell, variant):
    for figure in amc.FIGURES:
        if cell.family == "model_grad":
            ref = amc.model_grad_reference(amc.model_grad_case(cell.nx, cell.nu, cell.order, variant), figure)
        else:
            ref = amc.plant_grad_reference(amc.plant_grad_case(cell.nx, cell.nu, cell.kind, variant), figure)
        print("%s %s %s: max|grad_ref| = %.3g" % (kv.aux_cell_id(cell), variant, figure, np.abs(ref["grad"]).max()))
        assert np.isfinite(ref["grad"]).all() and np.abs(ref["grad"]).max() > 1e-3


@pytest.mark.parametrize("variant", amc.VARIANTS)
@pytest.mark.parametrize("cell", [c for c in _cells("plant_linearize") if c.kind != kv.REFUSED], ids=kv.aux_cell_id)
def test_linearisation_inputs(cell, variant):
    ref = amc.plant_linearize_reference(amc.plant_linearize_case(cell.nx, cell.nu, cell.kind, variant))
    assert all(np.isfinite(r).all() for r in ref) and np.abs(ref[1]).max() > 1e-3


@pytest.mark.parametrize("variant", amc.VARIANTS)
@pytest.mark.parametrize("cell", _cells("model_feedback", "plant_feedback"), ids=kv.aux_cell_id)
def test_feedback_inputs(cell, variant):
    if cell.family == "model_feedback":
        c = amc.model_feedback_case(cell.nx, cell.nu, cell.order, variant)
        ref = amc.model_feedback_define(c)
    else:
        c = amc.plant_feedback_case(cell.nx, cell.nu, cell.kind, variant)
        ref = amc.plant_feedback_define(c)
    act = amc.feedback_activity(c["law"], ref)
    print("%s %s: %s" % (kv.aux_cell_id(cell), variant, act))
    assert np.array_equal(ref["status"], np.zeros(amc.B, np.int32))
    assert act["lower"] > 0 and act["upper"] > 0 and act["interior"] > 0 and act["band"] > 0, act
    assert (ref["margin"] >= 1e-9).any()                                                  # a member whose clip count is certain


@pytest.mark.parametrize("cell", [c for c in _cells(*kv.FIT_FAMILIES) if c.kind != kv.REFUSED], ids=kv.aux_cell_id)
def test_fit_inputs(cell):
    c = amc.fit_case(cell.nx, cell.nu, cell.order, cell.family.startswith("refit"))
    nz = kv.lifted_size(cell.nx, cell.nu, cell.order)
    assert c["svals"].shape == (amc.FIT_B, nz) and c["A"].shape[1:] == (amc.FIT_B, cell.nx, nz)
    lo = fit.RCOND_MIN_QR if cell.family.endswith("qr") else fit.RCOND_MIN
    for r, rc in enumerate(c["rconds"]):
        ratio = c["svals"] / (rc * c["svals"][:, :1])
        assert np.all((ratio >= 1.2) | (ratio <= 1 / 1.2)) and np.array_equal(c["rank"][r], (ratio > 1).sum(axis=1))
        assert lo <= rc < 1
    assert (c["rank"] < nz).any() and np.all(c["rank"] >= 1)
    gram, qr = gram_bounds(c).max(axis=1), qr_bounds(c).max(axis=1)
    print("%s: cut-offs %s, ranks %s, Gram bounds %s, QR bounds %s" % (kv.aux_cell_id(cell), c["rconds"], c["rank"].tolist(), gram, qr))
    assert gram.min() <= 1e-8


@pytest.mark.parametrize("cell", [c for c in _cells("online") if c.kind != kv.REFUSED], ids=kv.aux_cell_id)
def test_online_inputs(cell):
    args = amc.online_args(cell.nx, cell.nu, cell.order, cell.kind == kv.HERMITIAN_FORM)
    want = amc.online_reference(args)
    s = sensitivity(args, want)
    print("%s: s = %s" % (kv.aux_cell_id(cell), s))
    assert np.all(want["status"] == 0) and np.all(s <= 1e-11), s
    cut = amc.online_args(cell.nx, cell.nu, cell.order, cell.kind == kv.HERMITIAN_FORM, E=2)
    assert cut["xs"].shape == (amc.B, 2, amc.ONLINE_N // 2 + 1, cell.nx) and cut["us"].shape == (2, amc.ONLINE_N // 2, cell.nu)
    assert np.array_equal(cut["xs"][:, 0, -1], cut["xs"][:, 1, 0])                        # the halves share a state

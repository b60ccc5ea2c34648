"""CPU checks of the batched DMDc fit (m4q_dmdc_fit_batch; mpc4quantum_amd/fit.py): the NumPy definition dmdc_fit_reference
against what the reference's DiscrepDMDc.from_data gave for the same data (tests/golden/dmdc_fit.npz, made by
tests/golden/make_golden_dmdc_fit.py), every refusal of the C ABI with its code before a device is asked for, and ValueError from
the Python wrappers before the library is touched.

Bound on a model: |A - A_ref| <= max(1e-13, 10 eps kappa_r^2) max(1, |A_ref|_inf), kappa_r = s_0 / s_r from the fixture's singular
values (r = the rank kept): the forward error of a normal-equations solve, whose Gram matrix has condition kappa^2."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, fit

DP, IP = _lib._dp, _lib._ip
EPS = np.finfo(np.float64).eps
CASES = "abcde"


def load_case(golden, name):
    g = golden("dmdc_fit")
    case = {k: g["%s_%s" % (name, k)] for k in ("xs", "us", "rconds", "A", "svals", "rank", "sens")}
    case["order"] = int(g[name + "_order"])
    case["u_scale"] = g[name + "_u_scale"] if name + "_u_scale" in g.files else None
    return case


def model_bounds(case):
    """[R, B]: the bound of the module docstring for every (rcond, member)."""
    sv, rank, A = case["svals"], case["rank"], case["A"]
    members = np.arange(sv.shape[0])
    kappa = sv[:, 0][None, :] / sv[members[None, :], rank - 1]
    return np.maximum(1e-13, 10 * EPS * kappa ** 2) * np.maximum(1.0, np.abs(A).max(axis=(2, 3)))


def worst_over_bound(models, case):
    return float((np.abs(models - case["A"]).max(axis=(2, 3)) / model_bounds(case)).max())


@pytest.fixture(scope="module")
def mirrored(golden):
    """dmdc_fit_reference on every fixture case, computed once."""
    out = {}
    for name in CASES:
        c = load_case(golden, name)
        out[name] = (c, fit.dmdc_fit_reference(c["xs"], c["us"], c["order"], c["rconds"], c["u_scale"]))
    return out


@pytest.mark.parametrize("name", CASES)
def test_fixture_keeps_its_margins(golden, name):
    """What make_golden_dmdc_fit.py asserted when it chose the cut-offs: each is a factor 1.2 from every singular value, and the
    case sees at least two ranks."""
    c = load_case(golden, name)
    for r, rc in enumerate(c["rconds"]):
        ratio = c["svals"] / (rc * c["svals"][:, :1])
        assert np.all((ratio >= 1.2) | (ratio <= 1 / 1.2))
        assert np.array_equal(c["rank"][r], (ratio > 1).sum(axis=1))
        assert fit.RCOND_MIN <= rc < 1
    assert len(np.unique(c["rank"])) >= 2


@pytest.mark.parametrize("name", CASES)
def test_definition_matches_the_reference_fit(mirrored, name, record_property):
    c, out = mirrored[name]
    assert np.array_equal(out["rank"], c["rank"])
    assert np.all(out["status"] == 0)
    worst = worst_over_bound(out["models"], c)
    record_property("worst_error_over_bound", worst)
    print("case %s: worst |A - A_ref| / bound = %.3g" % (name, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name", CASES)
def test_definition_singular_values(mirrored, name):
    """svals to 1e-12 s_0 against the SVD of the data, the two null singular values of case a included (what the device test asks
    of the kernel): they come from the snapshots through the eigenvectors, not from the eigenvalues of G."""
    c, out = mirrored[name]
    err = np.abs(out["svals"] - c["svals"]).max(axis=1) / c["svals"][:, 0]
    print("case %s: max |s - s_ref| / s_0 per member = %s" % (name, err))
    assert np.all(np.diff(out["svals"], axis=1) <= 0)
    assert np.all(err <= 1e-12)


@pytest.mark.parametrize("name", CASES)
def test_definition_converges_within_15_sweeps(mirrored, name):
    """A condition on the inputs: the cap of 30 is never why a case passes."""
    _, out = mirrored[name]
    print("case %s: sweeps %s" % (name, out["sweeps"]))
    assert np.all(out["sweeps"] <= 15)


def test_jacobi_decomposes_a_hermitian_matrix():
    rng = np.random.default_rng(5)
    M = rng.standard_normal((7, 11)) + 1j * rng.standard_normal((7, 11))
    G = M @ M.conj().T
    lam, V, sweeps, converged = fit.jacobi_hermitian(G)
    assert converged and sweeps <= 15
    assert np.abs(V.conj().T @ V - np.eye(7)).max() < 1e-14
    assert np.abs((V * lam) @ V.conj().T - G).max() < 1e-13 * np.abs(G).max()
    assert np.allclose(np.sort(lam), np.linalg.eigvalsh(G), rtol=1e-12)


def test_lifted_controls_follow_the_model_wrapper():
    rng = np.random.default_rng(6)
    for m, order in ((1, 1), (2, 1), (3, 1), (1, 2), (2, 2), (1, 4)):
        P = m4q.size_of_library(order, m) - 1
        u = rng.standard_normal((5, m))
        wrap = m4q.WrapModel(np.zeros((2, 2)), np.zeros((2, 2 * P)), m, order)
        assert np.allclose(fit.lift_controls(u, order), wrap.lift_u(u.T).T, rtol=1e-14, atol=0)


def test_non_finite_data_give_status_3():
    rng = np.random.default_rng(7)
    xs = rng.standard_normal((3, 6, 4)) + 0j
    us = rng.standard_normal((5, 1))
    clean = fit.dmdc_fit_reference(xs, us, 1, 1e-3)
    xs[1, 2, 3] = np.nan
    out = fit.dmdc_fit_reference(xs, us, 1, 1e-3)
    assert list(out["status"]) == [0, 3, 0] and out["rank"][1] == 0 and not out["models"][1].any() and not out["svals"][1].any()
    for b in (0, 2):
        assert np.array_equal(out["models"][b], clean["models"][b])


# ---------------------------------------------------------------- the C ABI
class _FitCall:
    """One valid m4q_dmdc_fit_batch call on host buffers of the right sizes; fields are replaced one at a time."""

    def __init__(self, B=3, n=9, m=2, order=1, E=2, N=4, P=2, R=3):
        nz = n * (1 + P)
        self.keep = {}
        rconds = np.full(max(R, 1), 1e-3)
        self.keep["rconds"] = rconds
        self.v = dict(B=B, n=n, m=m, order=order, E=E, N=N, xs=self._b("xs", 2 * B * E * (N + 1) * n), u=self._b("u", E * N * m), u_per=0,
                      u_scale=None, rconds=rconds.ctypes.data_as(DP), R=R, models=self._b("models", 2 * R * B * n * nz),
                      ranks=self._i("ranks", R * B), svals=self._b("svals", B * nz), status=self._i("status", B))

    def _b(self, name, count):
        self.keep[name] = np.zeros(max(int(count), 1), dtype=np.float64)
        return self.keep[name].ctypes.data_as(DP)

    def _i(self, name, count):
        self.keep[name] = np.zeros(max(int(count), 1), dtype=np.int32)
        return self.keep[name].ctypes.data_as(IP)

    def __call__(self, rcond=None, **change):
        v = dict(self.v, **change)
        if rcond is not None:
            self.keep["rconds"][:] = 1e-3
            self.keep["rconds"][min(1, len(self.keep["rconds"]) - 1)] = rcond
        return _lib.lib().m4q_dmdc_fit_batch(v["B"], v["n"], v["m"], v["order"], v["E"], v["N"], v["xs"], v["u"], v["u_per"],
                                             v["u_scale"], v["rconds"], v["R"], v["models"], v["ranks"], v["svals"], v["status"])


@pytest.mark.parametrize("change", [dict(B=0), dict(B=-1), dict(E=0), dict(E=-3), dict(N=0), dict(N=-1), dict(R=0), dict(R=-1),
                                    dict(R=17), dict(xs=None), dict(u=None), dict(rconds=None), dict(models=None), dict(status=None),
                                    dict(rcond=0.0), dict(rcond=1e-15), dict(rcond=9.99e-8), dict(rcond=1.0), dict(rcond=2.0),
                                    dict(rcond=-1e-3), dict(rcond=float("nan")), dict(rcond=float("inf"))], ids=str)
def test_fit_refuses_bad_arguments(change):
    assert _FitCall()(**change) == _lib.E_BADARG
    assert _lib.lib().m4q_last_error()


def test_fit_refuses_shapes_without_a_kernel():
    assert _FitCall(n=25)() == _lib.E_UNSUPPORTED                              # no compiled shape
    assert _FitCall(n=9, order=3, P=9)() == _lib.E_UNSUPPORTED
    assert _FitCall(n=16, m=2, order=1, P=2)() == _lib.E_UNSUPPORTED           # the plant-only shape has no model
    assert _FitCall(n=16, m=1, order=4, P=4)() == _lib.E_UNSUPPORTED           # nz = 80: the layout does not fit the LDS
    assert b"LDS" in _lib.lib().m4q_last_error()


def test_valid_fit_calls_need_a_device():
    """The range ends, the optional outputs left out and every supported shape get as far as asking for a device."""
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    assert _FitCall()() == _lib.E_NODEVICE
    assert _FitCall()(rcond=1e-7) == _lib.E_NODEVICE
    assert _FitCall()(rcond=0.999) == _lib.E_NODEVICE
    assert _FitCall(R=16)() == _lib.E_NODEVICE
    assert _FitCall()(ranks=None, svals=None) == _lib.E_NODEVICE
    for n, m, order, P in ((4, 1, 1, 1), (4, 1, 2, 2), (4, 2, 1, 2), (9, 2, 2, 5), (16, 3, 1, 3), (16, 1, 1, 1), (16, 1, 2, 2),
                           (16, 1, 3, 3), (8, 2, 1, 2)):
        assert _FitCall(n=n, m=m, order=order, P=P)() == _lib.E_NODEVICE, (n, m, order)
    with pytest.raises(_lib.M4qError):
        m4q.dmdc_fit_batch(np.zeros((2, 5, 4)), np.zeros((4, 1)), 1, 1e-3)


# ---------------------------------------------------------------- the Python wrappers
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was touched before the shapes were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _args(B=3, E=2, N=4, n=9, m=2):
    return dict(xs=np.zeros((B, E, N + 1, n), complex), us=np.zeros((E, N, m)), order=1, rcond=1e-3)


FIT_BAD = [dict(xs=np.zeros((3, 9))), dict(xs=np.zeros((3, 2, 5, 9, 1))), dict(xs=np.zeros((3, 2, 1, 9))), dict(xs=np.zeros((0, 2, 5, 9))),
           dict(us=np.zeros(4)), dict(us=np.zeros((2, 5, 2))), dict(us=np.zeros((3, 4, 2))), dict(us=np.zeros((2, 2, 4, 2))),
           dict(us=np.zeros((3, 2, 4, 2, 1))), dict(us=np.zeros((2, 4, 0))), dict(order=0), dict(u_scale=np.ones(2)),
           dict(u_scale=np.ones((3, 1))), dict(u_scale=np.ones((2, 2))), dict(rcond=1e-15), dict(rcond=0.0), dict(rcond=1.0),
           dict(rcond=[1e-3, 1e-8]), dict(rcond=np.float64("nan")), dict(rcond=[]), dict(rcond=np.full(17, 1e-3)),
           dict(rcond=np.full((2, 2), 1e-3))]


@pytest.mark.parametrize("change", FIT_BAD, ids=lambda c: ",".join("%s%s" % (k, getattr(v, "shape", v)) for k, v in c.items()))
def test_fit_wrappers_refuse_malformed_calls(no_library, change):
    args = dict(_args(), **change)
    with pytest.raises(ValueError):
        m4q.dmdc_fit_batch(**args)
    with pytest.raises(ValueError):
        fit.dmdc_fit_reference(**args)
    args["rconds"] = args.pop("rcond")
    with pytest.raises(ValueError):
        m4q.train_models_batch(**args)


def test_wrapper_hands_the_kernel_what_it_was_given(monkeypatch):
    seen = {}

    class Fake:
        def m4q_dmdc_fit_batch(self, *a):
            seen["a"] = a
            return 0

        def m4q_last_error(self):
            return b""
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    B, E, N, n, m = 3, 2, 4, 9, 2
    out = m4q.dmdc_fit_batch(np.zeros((B, E, N + 1, n)), np.zeros((E, N, m)), 1, [1e-3, 1e-2], u_scale=np.ones((B, m)))
    a = seen["a"]
    assert a[:6] == (B, n, m, 1, E, N) and a[8] == 0 and a[9] is not None and a[11] == 2
    assert np.array_equal(np.ctypeslib.as_array(a[10], (2,)), [1e-3, 1e-2])
    assert out["models"].shape == (2, B, n, 27) and out["rank"].shape == (2, B) and out["svals"].shape == (B, 27)
    assert out["status"].shape == (B,)
    out = m4q.dmdc_fit_batch(np.zeros((B, N + 1, n)), np.zeros((B, N, m)), 1, 1e-3)          # E = 1, per-member controls, scalar rcond
    a = seen["a"]
    assert a[:6] == (B, n, m, 1, 1, N) and a[8] == 1 and a[9] is None and a[11] == 1
    assert out["models"].shape == (B, n, 27) and out["rank"].shape == (B,)


def test_prototype_and_exports():
    assert len(_lib.PROTOTYPES["m4q_dmdc_fit_batch"][1]) == 16
    assert m4q.dmdc_fit_batch is fit.dmdc_fit_batch and m4q.train_models_batch is fit.train_models_batch
    assert m4q.dmdc_fit_reference is fit.dmdc_fit_reference

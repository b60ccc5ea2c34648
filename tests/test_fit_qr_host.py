"""CPU checks of the QR route of the batched DMDc fit (m4q_dmdc_fit_qr_batch; mpc4quantum_amd/fit.py): the NumPy definition
dmdc_fit_qr_reference against what the reference's DiscrepDMDc.from_data gave for the same ill-conditioned data
(tests/golden/dmdc_fit_qr.npz, made by tests/golden/make_golden_dmdc_fit_qr.py), what the Gram route makes of them, every refusal of
the C ABI with its code before a device is asked for, and ValueError from the Python wrappers before the library is touched.

Bound on a model, wherever a fit meets the reference's A: |A - A_ref|_inf <= max(1e-13 max(1, |A_ref|_inf), 100 sens), sens being
how far the reference's own A moves under a relative 1e-15 jitter of the data (the largest of three draws, which see three
directions and underestimate the worst case: hence the factor 100, the rule of tests/test_gpu_online.py)."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, fit
from tests.test_fit_host import _FitCall, _args, no_library  # noqa: F401  (no_library is a fixture)

CASES = "pqrs"
SHAPES = {"p": (4, 1, 1, 8), "q": (9, 2, 1, 27), "r": (9, 2, 2, 54), "s": (16, 3, 1, 64)}


def load_case(golden, name):
    g = golden("dmdc_fit_qr")
    case = {k: g["%s_%s" % (name, k)] for k in ("xs", "us", "u_scale", "rconds", "A", "svals", "rank", "sens")}
    case["order"] = int(g[name + "_order"])
    return case


def model_bounds(case):
    """[R, B]: the bound of the module docstring for every (rcond, member)."""
    return np.maximum(1e-13 * np.maximum(1.0, np.abs(case["A"]).max(axis=(2, 3))), 100 * case["sens"])


def model_errors(models, case):
    return np.abs(models - case["A"]).max(axis=(2, 3))


def kappas(case):
    """[R, B]: s_0 / s_rank of the data at every cut-off."""
    sv = case["svals"]
    return sv[:, 0][None, :] / sv[np.arange(sv.shape[0])[None, :], case["rank"] - 1]


def report(what, name, err, bound, record_property):
    """Print and record every measured error with its bound; returns the worst ratio."""
    for r in range(err.shape[0]):
        for b in range(err.shape[1]):
            print("case %s cut-off %d member %d: %s = %.3g, bound %.3g" % (name, r, b, what, err[r, b], bound[r, b]))
            record_property("%s_%s_r%d_b%d" % (what.replace(" ", "_"), name, r, b), (float(err[r, b]), float(bound[r, b])))
    return float((err / bound).max())


@pytest.fixture(scope="module")
def defined(golden):
    """dmdc_fit_qr_reference on every fixture case, computed once."""
    out = {}
    for name in CASES:
        c = load_case(golden, name)
        out[name] = (c, fit.dmdc_fit_qr_reference(c["xs"], c["us"], c["order"], c["rconds"], c["u_scale"]))
    return out


@pytest.mark.parametrize("name", CASES)
def test_fixture_keeps_its_margins(golden, name):
    """What make_golden_dmdc_fit_qr.py asserted when it chose the cut-offs."""
    c = load_case(golden, name)
    n, m, order, nz = SHAPES[name]
    assert c["xs"].shape[0] == 2 and c["xs"].shape[2:] == (41, n) and c["us"].shape[1:] == (40, m) and c["order"] == order
    assert c["u_scale"].shape == (2, m) and c["svals"].shape == (2, nz)
    for r, rc in enumerate(c["rconds"]):
        ratio = c["svals"] / (rc * c["svals"][:, :1])
        assert np.all((ratio >= 1.2) | (ratio <= 1 / 1.2))
        assert np.array_equal(c["rank"][r], (ratio > 1).sum(axis=1))
        assert 1e-10 * (1 - 1e-12) <= rc <= 1e-1 * (1 + 1e-12) and fit.RCOND_MIN_QR <= rc < 1
    assert len(np.unique(c["rank"])) >= 2
    if name in "qs":
        assert c["rconds"].min() <= 1e-8
    assert np.all(c["sens"] <= 1e-8 * np.maximum(1.0, np.abs(c["A"]).max(axis=(2, 3))))


def test_fixture_spans_the_range_and_holds_a_hard_cutoff(golden):
    rconds = np.concatenate([load_case(golden, name)["rconds"] for name in CASES])
    assert rconds.min() <= 1e-10 * (1 + 1e-12) and rconds.max() >= 1e-1 * (1 - 1e-12)
    assert max(kappas(load_case(golden, name)).max() for name in CASES) >= 1e5


@pytest.mark.parametrize("name", CASES)
def test_definition_matches_the_reference_fit(defined, name, record_property):
    c, out = defined[name]
    assert np.array_equal(out["rank"], c["rank"])
    assert np.all(out["status"] == 0)
    worst = report("definition error", name, model_errors(out["models"], c), model_bounds(c), record_property)
    assert worst <= 1.0


@pytest.mark.parametrize("name", CASES)
def test_definition_singular_values(defined, name, record_property):
    c, out = defined[name]
    err = np.abs(out["svals"] - c["svals"]).max(axis=1) / c["svals"][:, 0]
    record_property("worst_sval_error_over_s0", float(err.max()))
    print("case %s: max |s - s_ref| / s_0 per member = %s" % (name, err))
    assert np.all(np.diff(out["svals"], axis=1) <= 0)
    assert np.all(err <= 1e-12)


@pytest.mark.parametrize("name", CASES)
def test_definition_converges_within_20_sweeps(defined, name):
    """A condition on the inputs: the cap of 30 is never why a case passes."""
    _, out = defined[name]
    print("case %s: sweeps %s" % (name, out["sweeps"]))
    assert np.all(out["sweeps"] <= 20)


def test_gram_route_misses_the_bound_where_the_data_are_ill_conditioned(golden, record_property):
    """Why the QR route exists, kept as a fact about the inputs: at every cut-off that the Gram route accepts (>= 1e-7) and whose
    kappa_r is at least 1e5 - there is at least one - dmdc_fit_reference misses the bound by a factor of 100 or more."""
    seen = 0
    for name in CASES:
        c = load_case(golden, name)
        hard = (c["rconds"] >= fit.RCOND_MIN) & (kappas(c).min(axis=1) >= 1e5)
        if not hard.any():
            continue
        sub = {k: c[k][hard] for k in ("A", "sens")}
        out = fit.dmdc_fit_reference(c["xs"], c["us"], c["order"], c["rconds"][hard], c["u_scale"])
        err, bound = model_errors(out["models"], sub), model_bounds(sub)
        report("gram error", name, err, bound, record_property)
        assert np.all(err.max(axis=1) >= 100 * bound.max(axis=1)), (name, err, bound)
        seen += int(hard.sum())
    assert seen >= 1


def test_jacobi_one_sided_decomposes_a_triangular_factor():
    rng = np.random.default_rng(8)
    R = np.triu(rng.standard_normal((9, 9)) + 1j * rng.standard_normal((9, 9)))
    M, V, sweeps, converged = fit.jacobi_one_sided(R)
    assert converged and sweeps <= 15
    assert np.abs(V.conj().T @ V - np.eye(9)).max() < 1e-14
    assert np.abs(R @ V - M).max() < 1e-13 * np.abs(R).max()
    gram = M.conj().T @ M
    assert np.abs(gram - np.diag(gram.diagonal())).max() < 1e-14 * np.abs(gram).max()
    assert np.allclose(np.sort(np.sqrt(gram.diagonal().real)), np.sort(np.linalg.svd(R, compute_uv=False)), rtol=1e-13)


def test_givens_qr_factors_the_stacked_data():
    rng = np.random.default_rng(9)
    Z = rng.standard_normal((6, 15)) + 1j * rng.standard_normal((6, 15))
    Y = rng.standard_normal((3, 15)) + 1j * rng.standard_normal((3, 15))
    R, T = fit.givens_qr(Z, Y)
    assert not np.tril(R, -1).any() and np.abs(R.diagonal().imag).max() < 1e-15 and np.all(R.diagonal().real > 0)
    assert np.abs(R.conj().T @ R - Z @ Z.conj().T).max() < 1e-13                       # R^H R = Z Z^H
    assert np.abs(T.conj().T @ R - Y @ Z.conj().T).max() < 1e-13                       # T^H R = Y Z^H
    assert fit.lane_sum(np.arange(27.0)) == 351.0


def test_non_finite_data_give_status_3():
    rng = np.random.default_rng(7)
    xs = rng.standard_normal((3, 11, 4)) + 0j
    us = rng.standard_normal((10, 1))
    clean = fit.dmdc_fit_qr_reference(xs, us, 1, 1e-3)
    assert list(clean["status"]) == [0, 0, 0] and np.all(clean["rank"] == 8)
    xs[1, 2, 3] = np.nan
    out = fit.dmdc_fit_qr_reference(xs, us, 1, 1e-3)
    assert list(out["status"]) == [0, 3, 0] and out["rank"][1] == 0 and not out["models"][1].any() and not out["svals"][1].any()
    for b in (0, 2):
        assert np.array_equal(out["models"][b], clean["models"][b])
    xs[1, 2, 3] = 0.0
    xs[2, 10, 0] = np.inf                                                           # in the last x_{t+1} alone
    assert list(fit.dmdc_fit_qr_reference(xs, us, 1, 1e-3)["status"]) == [0, 0, 3]


# ---------------------------------------------------------------- the C ABI
class _QrCall(_FitCall):
    """One valid m4q_dmdc_fit_qr_batch call on host buffers of the right sizes; fields are replaced one at a time."""

    def __call__(self, rcond=None, **change):
        v = dict(self.v, **change)
        if rcond is not None:
            self.keep["rconds"][:] = 1e-3
            self.keep["rconds"][min(1, len(self.keep["rconds"]) - 1)] = rcond
        return _lib.lib().m4q_dmdc_fit_qr_batch(v["B"], v["n"], v["m"], v["order"], v["E"], v["N"], v["xs"], v["u"], v["u_per"],
                                                v["u_scale"], v["rconds"], v["R"], v["models"], v["ranks"], v["svals"], v["status"])


@pytest.mark.parametrize("change", [dict(B=0), dict(B=-1), dict(E=0), dict(E=-3), dict(N=0), dict(N=-1), dict(R=0), dict(R=-1),
                                    dict(R=17), dict(xs=None), dict(u=None), dict(rconds=None), dict(models=None), dict(status=None),
                                    dict(rcond=0.0), dict(rcond=1e-15), dict(rcond=1e-13), dict(rcond=9.99e-13), dict(rcond=1.0),
                                    dict(rcond=2.0), dict(rcond=-1e-3), dict(rcond=float("nan")), dict(rcond=float("inf"))], ids=str)
def test_qr_fit_refuses_bad_arguments(change):
    assert _QrCall()(**change) == _lib.E_BADARG
    assert _lib.lib().m4q_last_error()


def test_qr_fit_refuses_shapes_without_a_kernel():
    assert _QrCall(n=25)() == _lib.E_UNSUPPORTED                              # no compiled shape
    assert _QrCall(n=9, order=3, P=9)() == _lib.E_UNSUPPORTED
    assert _QrCall(n=16, m=2, order=1, P=2)() == _lib.E_UNSUPPORTED           # the plant-only shape has no model
    assert _QrCall(n=16, m=1, order=4, P=4)() == _lib.E_UNSUPPORTED           # nz = 80: the layout does not fit the LDS
    assert b"LDS" in _lib.lib().m4q_last_error()


def test_valid_qr_fit_calls_need_a_device():
    """The range ends, the optional outputs left out and every supported shape get as far as asking for a device."""
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    assert _QrCall()() == _lib.E_NODEVICE
    assert _QrCall()(rcond=1e-12) == _lib.E_NODEVICE
    assert _QrCall()(rcond=1e-10) == _lib.E_NODEVICE
    assert _FitCall()(rcond=1e-10) == _lib.E_BADARG                           # the Gram route's range is unchanged
    assert _QrCall()(rcond=0.999) == _lib.E_NODEVICE
    assert _QrCall(R=16)() == _lib.E_NODEVICE
    assert _QrCall()(ranks=None, svals=None) == _lib.E_NODEVICE
    for n, m, order, P in ((4, 1, 1, 1), (4, 1, 2, 2), (4, 2, 1, 2), (9, 2, 2, 5), (16, 3, 1, 3), (16, 1, 1, 1), (16, 1, 2, 2),
                           (16, 1, 3, 3), (8, 2, 1, 2)):
        assert _QrCall(n=n, m=m, order=order, P=P)() == _lib.E_NODEVICE, (n, m, order)
    with pytest.raises(_lib.M4qError):
        m4q.dmdc_fit_batch(np.zeros((2, 5, 4)), np.zeros((4, 1)), 1, 1e-10, method="qr")


# ---------------------------------------------------------------- the Python wrappers
def test_rcond_1e_10_is_accepted_by_qr_and_refused_by_the_default(monkeypatch):
    seen = []

    class Fake:
        def m4q_dmdc_fit_qr_batch(self, *a):
            seen.append(("qr", a))
            return 0

        def m4q_dmdc_fit_batch(self, *a):
            seen.append(("gram", a))
            return 0

        def m4q_last_error(self):
            return b""
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    B, E, N, n, m = 3, 2, 4, 9, 2
    args = dict(_args(B, E, N, n, m), rcond=[1e-10, 1e-3], u_scale=np.ones((B, m)))
    out = m4q.dmdc_fit_batch(method="qr", **args)
    assert [s[0] for s in seen] == ["qr"]
    a = seen[0][1]
    assert a[:6] == (B, n, m, 1, E, N) and a[8] == 0 and a[9] is not None and a[11] == 2
    assert np.array_equal(np.ctypeslib.as_array(a[10], (2,)), [1e-10, 1e-3])
    assert out["models"].shape == (2, B, n, 27) and out["rank"].shape == (2, B) and out["svals"].shape == (B, 27)
    with pytest.raises(ValueError, match="Gram"):
        m4q.dmdc_fit_batch(**args)
    with pytest.raises(ValueError, match="Gram"):
        m4q.dmdc_fit_batch(method="gram", **args)
    assert [s[0] for s in seen] == ["qr"]
    m4q.dmdc_fit_batch(**dict(args, rcond=1e-3))
    assert [s[0] for s in seen] == ["qr", "gram"]
    fit.dmdc_fit_qr_reference(**dict(args, rcond=1e-10))                      # accepted (all-zero data: rank 0)
    with pytest.raises(ValueError):
        fit.dmdc_fit_reference(**dict(args, rcond=1e-10))


QR_BAD = [dict(rcond=1e-13), dict(rcond=1e-15), dict(rcond=1.0), dict(rcond=np.float64("nan")), dict(rcond=[1e-3, 1e-13]),
          dict(method="svd"), dict(method=None), dict(method="QR")]


@pytest.mark.parametrize("change", QR_BAD, ids=str)
def test_qr_wrappers_refuse_malformed_calls(no_library, change):  # noqa: F811
    args = dict(_args(), method="qr")
    args.update(change)
    with pytest.raises(ValueError):
        m4q.dmdc_fit_batch(**args)
    if "method" not in change:
        with pytest.raises(ValueError):
            fit.dmdc_fit_qr_reference(**{k: v for k, v in args.items() if k != "method"})
    args["rconds"] = args.pop("rcond")
    with pytest.raises(ValueError):
        m4q.train_models_batch(**args)


def test_the_1e_15_refusal_names_the_host_call(no_library):  # noqa: F811
    with pytest.raises(ValueError, match="1e-15.*DiscrepDMDc.from_data"):
        m4q.dmdc_fit_batch(**dict(_args(), rcond=1e-15, method="qr"))


def test_prototype_matches_the_header():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "m4q.h")).read()
    decl = {name: re.search(r"M4Q_API int %s\((.*?)\);" % name, header, re.S).group(1) for name in ("m4q_dmdc_fit_batch", "m4q_dmdc_fit_qr_batch")}
    squeeze = lambda text: re.sub(r"\s+", " ", text).strip()  # noqa: E731
    assert squeeze(decl["m4q_dmdc_fit_qr_batch"]) == squeeze(decl["m4q_dmdc_fit_batch"])          # exactly the Gram route's arguments
    assert _lib.PROTOTYPES["m4q_dmdc_fit_qr_batch"] == _lib.PROTOTYPES["m4q_dmdc_fit_batch"]
    assert len(_lib.PROTOTYPES["m4q_dmdc_fit_qr_batch"][1]) == len(decl["m4q_dmdc_fit_qr_batch"].split(",")) == 16
    assert re.search(r"#define M4Q_FIT_QR_RCOND_MIN 1e-12\b", header) and fit.RCOND_MIN_QR == 1e-12
    assert re.search(r"#define M4Q_FIT_RCOND_MIN 1e-7\b", header) and fit.RCOND_MIN == 1e-7
    assert m4q.dmdc_fit_qr_reference is fit.dmdc_fit_qr_reference

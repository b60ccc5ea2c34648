"""CPU checks of the DMDc fit against a prior model (m4q_dmdc_refit_batch, m4q_dmdc_refit_qr_batch; mpc4quantum_amd/fit.py: the
arguments A0, discount and counts): the two NumPy definitions against what ONE DiscrepDMDc.fit_iteration of the reference gave
(tests/golden/dmdc_refit.npz, made by tests/golden/make_golden_dmdc_refit.py) and against A0 + (Y - A0 Z) pinv(Z w, rcond) formed
with NumPy, the identities that tie them to the plain fit, every refusal of the two C entry points with its code before a device is
asked for, and ValueError from the Python wrappers before the library is touched.

Bounds, nothing new: the Gram route is held to tests/test_fit_host.py's max(1e-13, 10 eps kappa_r^2) max(1, |A|), the QR route to
tests/test_fit_qr_host.py's max(1e-13 max(1, |A|), 100 sens), both on this fixture's svals / rank / sens (those of the weighted
stack)."""
import os
import re

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, fit
from tests.test_fit_host import _FitCall, _args, model_bounds as gram_bounds, no_library  # noqa: F401  (no_library is a fixture)
from tests.test_fit_qr_host import model_bounds as qr_bounds

CASES = "abcde"
ROUTES = {"gram": (fit.dmdc_fit_reference, gram_bounds), "qr": (fit.dmdc_fit_qr_reference, qr_bounds)}
FIELDS = ("models", "rank", "svals", "status")


def load_case(golden, name):
    """The case's prior, cut-offs and the reference's update from dmdc_refit.npz; its data from there (case a) or dmdc_fit.npz."""
    g, data = golden("dmdc_refit"), golden("dmdc_fit")
    case = {k: g["%s_%s" % (name, k)] for k in ("A0", "counts", "rconds", "A", "svals", "rank", "sens")}
    case["discount"] = float(g[name + "_discount"])
    src = g if name + "_xs" in g.files else data
    case.update(xs=src[name + "_xs"], us=src[name + "_us"], order=int(src[name + "_order"]))
    case["u_scale"] = src[name + "_u_scale"] if name + "_u_scale" in src.files else None
    return case


def prior_args(c):
    return dict(xs=c["xs"], us=c["us"], order=c["order"], rcond=c["rconds"], u_scale=c["u_scale"], A0=c["A0"], discount=c["discount"],
                counts=c["counts"])


def weighted_stacks(c, b):
    """(Z, Y, w) of member b: the snapshots it takes and their weights discount^(S-1-s)."""
    us = c["us"][b] if c["us"].ndim == 4 else c["us"]
    if c["u_scale"] is not None:
        us = c["u_scale"][b] * us
    Z, Y = fit.stack_snapshots(c["xs"][b], us, c["order"])
    Z, Y = fit.taken_snapshots(Z, Y, c["xs"].shape[1], int(c["counts"][b]))
    return Z, Y, c["discount"] ** np.arange(Z.shape[1] - 1, -1, -1.0)


def closed_form(c):
    """A0 + (Y - A0 Z) pinv(Z, rcond) on the weighted stacks, [R, B, n, nz]."""
    out = np.zeros_like(c["A"])
    for b in range(c["xs"].shape[0]):
        Z, Y, w = weighted_stacks(c, b)
        for r, rc in enumerate(c["rconds"]):
            out[r, b] = c["A0"][b] + ((Y - c["A0"][b] @ Z) * w) @ np.linalg.pinv(Z * w, rcond=rc)
    return out


def worst(models, c, bounds, what, name, record_property):
    ratio = float((np.abs(models - c["A"]).max(axis=(2, 3)) / bounds(c)).max())
    record_property("worst_error_over_bound", ratio)
    print("case %s, %s: worst error / bound = %.3g, max error = %.3g" % (name, what, ratio, np.abs(models - c["A"]).max()))
    return ratio


@pytest.fixture(scope="module")
def defined(golden):
    """Both definitions on every fixture case, computed once."""
    out = {}
    for name in CASES:
        c = load_case(golden, name)
        out[name] = (c, {route: fn(**prior_args(c)) for route, (fn, _) in ROUTES.items()})
    return out


@pytest.mark.parametrize("name", CASES)
def test_fixture_keeps_what_its_script_asserted(golden, name):
    c = load_case(golden, name)
    nz = c["A"].shape[-1]
    for r, rc in enumerate(c["rconds"]):
        ratio = c["svals"] / (rc * c["svals"][:, :1])
        assert np.all((ratio >= 1.2) | (ratio <= 1 / 1.2))
        assert np.array_equal(c["rank"][r], (ratio > 1).sum(axis=1))
        assert fit.RCOND_MIN <= rc < 1
    assert (c["rank"] < nz).any()
    for b in range(c["xs"].shape[0]):
        Z, Y, w = weighted_stacks(c, b)
        assert np.linalg.matrix_rank(Z[:c["xs"].shape[-1]] * w) >= c["xs"].shape[-1]            # the reference's gate was open
        for r, rc in enumerate(c["rconds"]):
            if c["rank"][r, b] < nz:
                assert np.abs(c["A"][r, b] - (Y * w) @ np.linalg.pinv(Z * w, rcond=rc)).max() > 1e-3
    assert np.abs(c["A"] - c["A0"][None]).max() > 1e-3


def test_fixture_discounts_some_cases_and_one_is_ragged(golden):
    cases = [load_case(golden, name) for name in CASES]
    assert sum(c["discount"] == 0.9 for c in cases) >= 2 and any(c["discount"] == 1.0 for c in cases)
    ragged = [c for c in cases if len(set(c["counts"])) > 1]
    assert len(ragged) == 1 and ragged[0]["counts"].max() == ragged[0]["xs"].shape[2] - 1


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", CASES)
def test_definition_matches_the_reference_update(defined, name, route, record_property):
    c, outs = defined[name]
    out = outs[route]
    assert np.array_equal(out["rank"], c["rank"]) and np.all(out["status"] == 0)
    assert worst(out["models"], c, ROUTES[route][1], route + " against the reference", name, record_property) <= 1.0
    err = np.abs(out["svals"] - c["svals"]).max(axis=1) / c["svals"][:, 0]
    assert np.all(np.diff(out["svals"], axis=1) <= 0) and np.all(err <= 1e-12), err


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", CASES)
def test_definition_matches_the_closed_form(defined, name, route, record_property):
    c, outs = defined[name]
    assert worst(outs[route]["models"], dict(c, A=closed_form(c)), ROUTES[route][1], route + " against NumPy's pinv", name,
                 record_property) <= 1.0


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", "ac")
def test_identities_with_the_plain_definition(golden, name, route):
    """A0 = 0, an explicit discount of 1 and full counts each give the plain definition's numbers (a -0.0 may change its sign)."""
    c = load_case(golden, name)
    fn = ROUTES[route][0]
    plain = dict(xs=c["xs"], us=c["us"], order=c["order"], rcond=c["rconds"], u_scale=c["u_scale"])
    want = fn(**plain)
    B, N = c["xs"].shape[0], c["xs"].shape[2] - 1
    for extra in (dict(A0=np.zeros_like(c["A0"][0])), dict(A0=np.zeros_like(c["A0"])), dict(discount=1.0), dict(discount=np.ones(B)),
                  dict(counts=np.full(B, N)), dict(A0=np.zeros_like(c["A0"]), discount=1.0, counts=np.full(B, N))):
        got = fn(**plain, **extra)
        for f in FIELDS + ("sweeps",):
            assert np.array_equal(got[f], want[f]), (f, list(extra))


@pytest.mark.parametrize("route", ROUTES)
def test_a_member_without_snapshots_keeps_its_prior(golden, route):
    c = load_case(golden, "c")
    args = prior_args(c)
    full = ROUTES[route][0](**args)
    counts = c["counts"].copy()
    counts[1] = 0
    out = ROUTES[route][0](**dict(args, counts=counts))
    assert list(out["status"]) == [0, 0, 0] and not out["rank"][:, 1].any() and not out["svals"][1].any()
    assert np.array_equal(out["models"][:, 1], np.broadcast_to(c["A0"][1], out["models"][:, 1].shape))
    for b in (0, 2):
        assert np.array_equal(out["models"][:, b], full["models"][:, b])


@pytest.mark.parametrize("route", ROUTES)
def test_ragged_counts_equal_cut_trajectories(golden, route):
    c = load_case(golden, "c")
    out = ROUTES[route][0](**prior_args(c))
    for b, cnt in enumerate(c["counts"]):
        alone = ROUTES[route][0](c["xs"][b:b + 1, :, :cnt + 1], c["us"][:, :cnt], c["order"], c["rconds"], A0=c["A0"][b],
                                 discount=c["discount"])
        for f in FIELDS:
            assert np.array_equal(np.moveaxis(out[f], -1 if f == "status" else (0 if f == "svals" else 1), 0)[b],
                                  np.moveaxis(alone[f], -1 if f == "status" else (0 if f == "svals" else 1), 0)[0]), f


@pytest.mark.parametrize("route", ROUTES)
def test_non_finite_prior_or_data_give_status_3(golden, route):
    c = load_case(golden, "a")
    args = prior_args(c)
    clean = ROUTES[route][0](**args)
    A0 = c["A0"].copy()
    A0[1, 2, 5] = np.nan
    xs = c["xs"].copy()
    xs[2, 0, 3, 1] = np.inf
    out = ROUTES[route][0](**dict(args, A0=A0, xs=xs))
    assert list(out["status"]) == [0, 3, 3] and not out["models"][:, 1:].any() and not out["rank"][:, 1:].any()
    assert not out["svals"][1:].any() and np.array_equal(out["models"][:, 0], clean["models"][:, 0])


# ---------------------------------------------------------------- the C ABI
class _RefitCall(_FitCall):
    """One valid m4q_dmdc_refit_batch / m4q_dmdc_refit_qr_batch call on host buffers of the right sizes."""

    def __init__(self, entry="m4q_dmdc_refit_batch", **kw):
        super().__init__(**kw)
        v = self.v
        nz = v["n"] * (1 + kw.get("P", 2))
        self.entry = entry
        self.keep["discount"] = np.full(max(v["B"], 1), 0.9)
        self.keep["counts"] = np.full(max(v["B"], 1), max(v["N"], 0), dtype=np.int32)
        v.update(A0=self._b("A0", 2 * v["B"] * v["n"] * nz), A0_per=1, discount=self.keep["discount"].ctypes.data_as(_lib._dp),
                 discount_per=1, counts=self.keep["counts"].ctypes.data_as(_lib._ip))

    def __call__(self, rcond=None, discount_value=None, count_value=None, **change):
        v = dict(self.v, **change)
        if rcond is not None:
            self.keep["rconds"][:] = 1e-3
            self.keep["rconds"][min(1, len(self.keep["rconds"]) - 1)] = rcond
        if discount_value is not None:
            self.keep["discount"][0 if not v["discount_per"] else -1] = discount_value
        if count_value is not None:
            self.keep["counts"][-1] = count_value
        return getattr(_lib.lib(), self.entry)(v["B"], v["n"], v["m"], v["order"], v["E"], v["N"], v["xs"], v["u"], v["u_per"],
                                               v["u_scale"], v["rconds"], v["R"], v["models"], v["ranks"], v["svals"], v["status"],
                                               v["A0"], v["A0_per"], v["discount"], v["discount_per"], v["counts"])


ENTRIES = ("m4q_dmdc_refit_batch", "m4q_dmdc_refit_qr_batch")
REFUSED = [dict(B=0), dict(B=-1), dict(E=0), dict(N=0), dict(N=-1), dict(R=0), dict(R=17), dict(xs=None), dict(u=None), dict(rconds=None),
           dict(models=None), dict(status=None), dict(rcond=0.0), dict(rcond=1.0), dict(rcond=float("nan")), dict(rcond=1e-15),
           dict(A0=None), dict(discount=None), dict(discount_value=0.0), dict(discount_value=-0.5), dict(discount_value=1.0000001),
           dict(discount_value=float("nan")), dict(discount_value=float("inf")), dict(discount_value=0.0, discount_per=0),
           dict(count_value=-1), dict(count_value=5)]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("change", REFUSED, ids=str)
def test_refit_refuses_bad_arguments(entry, change):
    assert _RefitCall(entry)(**change) == _lib.E_BADARG
    assert entry.encode() in _lib.lib().m4q_last_error()


def test_refit_keeps_the_rcond_range_of_its_route():
    assert _RefitCall(ENTRIES[0])(rcond=9.99e-8) == _lib.E_BADARG and _RefitCall(ENTRIES[1])(rcond=9.99e-13) == _lib.E_BADARG
    assert _RefitCall(ENTRIES[1])(rcond=1e-10) != _lib.E_BADARG and _RefitCall(ENTRIES[0])(rcond=1e-7) != _lib.E_BADARG


@pytest.mark.parametrize("entry", ENTRIES)
def test_refit_refuses_shapes_without_a_kernel(entry):
    assert _RefitCall(entry, n=25)() == _lib.E_UNSUPPORTED                              # no compiled shape
    assert _RefitCall(entry, n=9, order=3, P=9)() == _lib.E_UNSUPPORTED
    assert _RefitCall(entry, n=16, m=2, order=1, P=2)() == _lib.E_UNSUPPORTED           # the plant-only shape has no model
    assert _RefitCall(entry, n=16, m=1, order=4, P=4)() == _lib.E_UNSUPPORTED           # nz = 80: the layout does not fit the LDS
    assert b"LDS" in _lib.lib().m4q_last_error()
    assert _RefitCall(entry, n=25)(A0=None) == _lib.E_UNSUPPORTED                       # as the fit: the shape is looked at first


@pytest.mark.parametrize("entry", ENTRIES)
def test_valid_refit_calls_need_a_device(entry):
    """The range ends, the optional arguments left out and every supported shape get as far as asking for a device."""
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    call = _RefitCall(entry)
    assert call() == _lib.E_NODEVICE
    assert call(counts=None) == _lib.E_NODEVICE and call(ranks=None, svals=None, u_scale=None) == _lib.E_NODEVICE
    assert call(A0_per=0, discount_per=0) == _lib.E_NODEVICE
    assert call(discount_value=1.0) == _lib.E_NODEVICE and call(discount_value=1e-300) == _lib.E_NODEVICE
    assert call(count_value=0) == _lib.E_NODEVICE and call(count_value=4) == _lib.E_NODEVICE
    for n, m, order, P in ((4, 1, 1, 1), (4, 1, 2, 2), (4, 2, 1, 2), (9, 2, 2, 5), (16, 3, 1, 3), (16, 1, 1, 1), (16, 1, 2, 2),
                           (16, 1, 3, 3), (8, 2, 1, 2)):
        assert _RefitCall(entry, n=n, m=m, order=order, P=P)() == _lib.E_NODEVICE, (n, m, order)
    with pytest.raises(_lib.M4qError):
        m4q.dmdc_fit_batch(np.zeros((2, 5, 4)), np.zeros((4, 1)), 1, 1e-3, A0=np.zeros((4, 8)),
                           method="qr" if entry.endswith("qr_batch") else "gram")


def test_prototypes_match_each_other_and_the_header():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "m4q.h")).read()
    names = ("m4q_dmdc_fit_batch",) + ENTRIES
    decl = {name: re.sub(r"\s+", " ", re.search(r"M4Q_API int %s\((.*?)\);" % name, header, re.S).group(1)).strip() for name in names}
    assert decl[ENTRIES[0]] == decl[ENTRIES[1]]
    assert decl[ENTRIES[0]] == decl["m4q_dmdc_fit_batch"] + (", const double* A0, int32_t A0_per_instance, const double* discount, "
                                                             "int32_t discount_per_instance, const int32_t* counts")
    assert _lib.PROTOTYPES[ENTRIES[0]] == _lib.PROTOTYPES[ENTRIES[1]]
    res, args = _lib.PROTOTYPES[ENTRIES[0]]
    assert (res, args[:16]) == _lib.PROTOTYPES["m4q_dmdc_fit_batch"] and len(args) == len(decl[ENTRIES[0]].split(",")) == 21
    assert args[16:] == [_lib._dp, _lib._i32, _lib._dp, _lib._i32, _lib._ip]
    assert m4q.refit_models_batch is fit.refit_models_batch


# ---------------------------------------------------------------- the Python wrappers
PRIOR_BAD = [dict(A0=np.zeros((9, 26))), dict(A0=np.zeros((2, 9, 27))), dict(A0=np.zeros((3, 9, 27, 1))), dict(A0=np.zeros(27)),
             dict(discount=0.0), dict(discount=1.5), dict(discount=-0.1), dict(discount=np.float64("nan")), dict(discount=np.ones(2)),
             dict(discount=np.ones((3, 1))), dict(discount=[0.9, 0.0, 0.9]), dict(counts=[4, 4]), dict(counts=4), dict(counts=[4, 5, 4]),
             dict(counts=[4, -1, 4]), dict(counts=[4.0, 4.0, 4.0]), dict(counts=np.ones((3, 1), dtype=int))]


@pytest.mark.parametrize("method", fit.METHODS)
@pytest.mark.parametrize("change", PRIOR_BAD, ids=lambda c: ",".join("%s%s" % (k, getattr(v, "shape", v)) for k, v in c.items()))
def test_wrappers_refuse_a_malformed_prior(no_library, change, method):  # noqa: F811
    args = dict(_args(), **change)
    with pytest.raises(ValueError):
        m4q.dmdc_fit_batch(method=method, **args)
    with pytest.raises(ValueError):
        ROUTES[method][0](**args)
    if "A0" in change:
        args["rconds"] = args.pop("rcond")
        with pytest.raises(ValueError):
            m4q.train_models_batch(method=method, **args)


def _run(B=3, n=4, m=1, ns=12, seed=3):
    rng = np.random.default_rng(seed)
    return {"xs": rng.standard_normal((B, ns + 1, n)) + 1j * rng.standard_normal((B, ns + 1, n)), "us": rng.standard_normal((B, ns, m)),
            "steps_done": np.array([ns, 9, 0][:B], dtype=np.int32)}


class _Clock:
    measure_freq = 1


def test_refit_of_a_run_refuses_malformed_calls(no_library):  # noqa: F811
    run, models = _run(), np.zeros((3, 4, 8), complex)

    class Sparse:
        measure_freq = 2
    for bad in (dict(clock=Sparse()), dict(models=np.zeros(8)), dict(models=np.zeros((2, 4, 8))), dict(models=np.zeros((3, 4, 12))),
                dict(rcond=1e-15), dict(discount=0.0), dict(method="svd"), dict(layout="time_first"),
                dict(run=dict(run, steps_done=np.array([13, 5, 0]))), dict(run=dict(run, us=run["us"][:, :-1]))):
        args = dict(dict(run=run, models=models, order=1, clock=_Clock(), rcond=1e-3), **bad)
        with pytest.raises(ValueError):
            m4q.refit_models_batch(**args)
        if "method" not in bad:
            with pytest.raises(ValueError):
                m4q.refit_models_batch(reference=True, **args)


@pytest.mark.parametrize("method", fit.METHODS)
def test_refit_of_a_run_is_one_update_per_member(method):
    """Both layouts of a run, counts = steps_done and A0 = models: the definition on each member's own steps."""
    run = _run()
    rng = np.random.default_rng(4)
    models = 0.2 * (rng.standard_normal((3, 4, 8)) + 1j * rng.standard_normal((3, 4, 8)))
    out = m4q.refit_models_batch(run, models, 1, _Clock(), [1e-3, 0.3], discount=0.95, method=method, reference=True)
    last = {"xs": np.swapaxes(run["xs"], 1, 2), "us": np.swapaxes(run["us"], 1, 2), "steps_done": run["steps_done"]}
    same = m4q.refit_models_batch(last, models, 1, _Clock(), [1e-3, 0.3], discount=0.95, method=method, layout="time_last", reference=True)
    assert list(out["status"]) == [0, 0, 0] and np.array_equal(out["models"][:, 2], np.stack([models[2]] * 2))
    for f in FIELDS:
        assert np.array_equal(out[f], same[f])
    for b, steps in enumerate(run["steps_done"][:2]):
        Z, Y = fit.stack_snapshots(run["xs"][b:b + 1, :steps + 1][0][None], run["us"][b, :steps][None], 1)
        w = 0.95 ** np.arange(steps - 1, -1, -1.0)
        for r, rc in enumerate((1e-3, 0.3)):
            want = models[b] + ((Y - models[b] @ Z) * w) @ np.linalg.pinv(Z * w, rcond=rc)
            assert np.abs(out["models"][r, b] - want).max() <= 1e-10 * max(1.0, np.abs(want).max())


def test_wrapper_hands_the_kernels_what_it_was_given(monkeypatch):
    seen = []

    class Fake:
        def __getattr__(self, name):
            if name == "m4q_last_error":
                return lambda: b""

            def call(*a):
                seen.append((name, a))
                return 0
            return call
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    B, E, N, n, m = 3, 2, 4, 9, 2
    base = _args(B, E, N, n, m)
    m4q.dmdc_fit_batch(**base)
    m4q.dmdc_fit_batch(method="qr", **base)
    assert [s[0] for s in seen] == ["m4q_dmdc_fit_batch", "m4q_dmdc_fit_qr_batch"] and all(len(s[1]) == 16 for s in seen)
    del seen[:]
    A0 = np.arange(B * n * 27).reshape(B, n, 27) + 0j
    m4q.dmdc_fit_batch(A0=A0, discount=[0.9, 0.8, 1.0], counts=[4, 0, 2], **base)
    m4q.dmdc_fit_batch(method="qr", A0=A0[0], **base)
    m4q.dmdc_fit_batch(discount=0.5, **base)
    m4q.dmdc_fit_batch(counts=np.array([1, 2, 3]), **base)
    assert [s[0] for s in seen] == ["m4q_dmdc_refit_batch", "m4q_dmdc_refit_qr_batch", "m4q_dmdc_refit_batch", "m4q_dmdc_refit_batch"]
    a = seen[0][1]
    assert len(a) == 21 and a[:6] == (B, n, m, 1, E, N) and a[17] == 1 and a[19] == 1
    assert np.array_equal(np.ctypeslib.as_array(a[16], (2 * B * n * 27,))[::2], np.arange(B * n * 27))
    assert np.array_equal(np.ctypeslib.as_array(a[18], (B,)), [0.9, 0.8, 1.0]) and np.array_equal(np.ctypeslib.as_array(a[20], (B,)), [4, 0, 2])
    a = seen[1][1]
    assert a[17] == 0 and a[19] == 0 and a[20] is None and np.ctypeslib.as_array(a[18], (1,))[0] == 1.0
    a = seen[2][1]
    assert a[17] == 0 and not np.ctypeslib.as_array(a[16], (2 * n * 27,)).any() and np.ctypeslib.as_array(a[18], (1,))[0] == 0.5
    assert np.array_equal(np.ctypeslib.as_array(seen[3][1][20], (B,)), [1, 2, 3])
    del seen[:]
    run = _run(B=3, n=9, m=2)
    m4q.refit_models_batch(run, A0, 1, _Clock(), 1e-3, discount=0.9, method="qr")
    name, a = seen[0]
    assert name == "m4q_dmdc_refit_qr_batch" and a[:6] == (3, 9, 2, 1, 1, 12) and a[8] == 1 and a[17] == 1 and a[19] == 0
    assert np.array_equal(np.ctypeslib.as_array(a[20], (3,)), run["steps_done"])


def test_training_against_a_prior_picks_what_a_host_loop_picks(golden, monkeypatch):
    """train_models_batch(A0=) with the device calls replaced by their definitions: every fit of the grid is made against the
    prior, and each member keeps the first cut-off that loses least along its training controls."""
    c = load_case(golden, "c")
    xs, us, order, A0 = c["xs"], c["us"], c["order"], c["A0"]
    B, E, N1, n = xs.shape
    grid = np.array([1e-4, 1e-2, 1e-1, 3e-1])

    def rollout(x0, u, models, order, u_scale=None, keep="all"):
        out = np.zeros((x0.shape[0], u.shape[-2] + 1, n), complex)
        out[:, 0] = x0
        for b in range(x0.shape[0]):
            pu = fit.lift_controls(u if u.ndim == 2 else u[b], order)
            for t in range(u.shape[-2]):
                z = np.concatenate([out[b, t]] + [p * out[b, t] for p in pu[t]])
                out[b, t + 1] = models[b] @ z
        return {"xs": out}
    calls = []

    def device_fit(xs, us, order, rcond, u_scale=None, method="gram", **prior):
        calls.append(prior)
        return fit.dmdc_fit_reference(xs, us, order, rcond, u_scale, **prior)
    monkeypatch.setattr(fit, "model_rollout_batch", rollout)
    monkeypatch.setattr(fit, "dmdc_fit_batch", device_fit)
    got = m4q.train_models_batch(xs, us, order, rconds=grid, A0=A0)
    assert len(calls) == 1 and calls[0]["A0"] is A0
    want = fit.dmdc_fit_reference(xs, us, order, grid, A0=A0)["models"]
    for b in range(B):
        losses = [sum(np.linalg.norm(xs[b, e, 1:] - rollout(xs[b:b + 1, e, 0], us[e], want[r, b:b + 1], order)["xs"][0, 1:], 2)
                      for e in range(E)) for r in range(len(grid))]
        assert got["index"][b] == int(np.argmin(losses)) and got["rcond"][b] == grid[got["index"][b]]
        assert np.array_equal(got["models"][b], want[got["index"][b], b])
    plain = m4q.train_models_batch(xs, us, order, rconds=grid)
    assert "A0" in calls[1] and calls[1]["A0"] is None and not np.array_equal(plain["models"], got["models"])

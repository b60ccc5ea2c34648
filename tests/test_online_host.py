"""CPU checks of the batched recursive DMDc update (m4q_online_dmdc_batch; mpc4quantum_amd/online.py): the NumPy definition
online_dmdc_reference against the product's OnlineDMDc and against what the reference's OnlineDMDc made of the same data
(tests/golden/online_dmdc.npz, made by tests/golden/make_golden_online_dmdc.py), against the closed form of the recursion, which
does not recurse, every refusal of the C ABI with its code before a device is asked for, and ValueError from the Python layer before
the library is touched.

The cases are (n, m, order, N, discount) with alpha = 1e2: a (4, 1, 1, 12, 1.0), b (4, 1, 1, 12, 0.95), c (9, 2, 1, 40, 0.97),
d (16, 3, 1, 40, 0.98), e (16, 1, 1, 24, 0.95).  Errors are relative to each member's max |A| or max |P|."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, fit, online

DP, IP = _lib._dp, _lib._ip
CASES = {"a": (4, 1, 1, 12, 1.0), "b": (4, 1, 1, 12, 0.95), "c": (9, 2, 1, 40, 0.97), "d": (16, 3, 1, 40, 0.98),
         "e": (16, 1, 1, 24, 0.95)}
ALPHA = 1e2
KEYS = ("xs", "us", "u_scale", "A0", "alpha", "discount", "order", "A_hist", "A", "P")


def load_case(golden, name):
    """One fixture case; xs [B, 1, N + 1, n] (E = 1)."""
    g = golden("online_dmdc")
    c = {k: g["%s_%s" % (name, k)] for k in KEYS}
    c["order"], c["alpha"], c["discount"] = int(c["order"]), float(c["alpha"]), float(c["discount"])
    c["xs"] = c["xs"][:, None]
    n, m, order, N, discount = CASES[name]
    assert c["xs"].shape[2:] == (N + 1, n) and c["us"].shape == (N, m) and c["order"] == order
    assert c["discount"] == discount and c["alpha"] == ALPHA
    return c


def two_experiments(c):
    """The same snapshots as E = 2 experiments of N / 2 steps: the trajectory cut in the middle (the halves share a state)."""
    N = c["us"].shape[0]
    h = N // 2
    xs = np.ascontiguousarray(np.stack([c["xs"][:, 0, :h + 1], c["xs"][:, 0, h:]], axis=1))
    return dict(c, xs=xs, us=np.ascontiguousarray(np.stack([c["us"][:h], c["us"][h:]])))


def call_args(c, **kw):
    args = dict(xs=c["xs"], us=c["us"], order=c["order"], A0=c["A0"], alpha=c["alpha"], discount=c["discount"], u_scale=c["u_scale"])
    args.update(kw)
    return args


def rel_err(got, want, scale_of=None):
    """max over members of max |got - want| / max |scale_of| per member (the ensemble axis is the one before the last two)."""
    scale = np.abs(want if scale_of is None else scale_of).max(axis=(-2, -1))
    return float((np.abs(got - want).max(axis=(-2, -1)) / scale).max())


def random_case(name, seed, B=2, E=1):
    """Unit-norm random states, controls in [-1, 1], a random A0 of size 0.1: the data the closed form was measured on."""
    n, m, order, N, discount = CASES[name]
    rng = np.random.default_rng([seed, ord(name)])
    xs = rng.standard_normal((B, E, N // E + 1, n)) + 1j * rng.standard_normal((B, E, N // E + 1, n))
    xs /= np.linalg.norm(xs, axis=-1, keepdims=True)
    nz = n * m4q.size_of_library(order, m)
    return dict(xs=xs, us=rng.uniform(-1, 1, (E, N // E, m)), order=order, alpha=ALPHA, discount=discount, u_scale=None,
                A0=0.1 * (rng.standard_normal((n, nz)) + 1j * rng.standard_normal((n, nz))))


def host_class_loop(c, b, steps=None, discount=None):
    """The product's OnlineDMDc fed with member b's snapshots one by one: (model, [A after each update])."""
    n, nz = c["A0"].shape[-2:]
    u = c["us"] if c["u_scale"] is None else c["u_scale"][b] * c["us"]
    Z, Y = fit.stack_snapshots(c["xs"][b], u.reshape(c["xs"].shape[1], -1, u.shape[-1]), c["order"])
    model = m4q.OnlineDMDc.from_bootstrap(n, n, nz - n, c["A0"].copy(), alpha=c["alpha"])
    model.discount = c["discount"] if discount is None else discount
    seen = []
    for k in range(Z.shape[1] if steps is None else steps):
        model.fit_iteration(Y[:, k], Z[:n, k], Z[n:, k])
        seen.append(model.A.copy())
    return model, seen


@pytest.fixture(scope="module")
def mirrored(golden):
    """online_dmdc_reference on every fixture case (hist_every = 5, innovations), computed once."""
    out = {}
    for name in CASES:
        c = load_case(golden, name)
        out[name] = (c, online.online_dmdc_reference(**call_args(c, hist_every=5, innovations=True)))
    return out


# ---------------------------------------------------------------- the definition against the classes
@pytest.mark.parametrize("name", CASES)
def test_definition_matches_the_reference_class(mirrored, name, record_property):
    c, out = mirrored[name]
    assert np.all(out["status"] == 0)
    eA, eP = rel_err(out["models"], c["A"]), rel_err(out["P"], c["P"])
    eH = rel_err(out["hist"], c["A_hist"], np.broadcast_to(c["A"], c["A_hist"].shape))
    record_property("rel_err_A", eA)
    record_property("rel_err_P", eP)
    print("case %s: A %.3g, P %.3g, hist %.3g" % (name, eA, eP, eH))
    assert out["hist"].shape == c["A_hist"].shape
    assert eA <= 1e-12 and eP <= 1e-12 and eH <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_definition_matches_the_host_class(mirrored, name):
    c, out = mirrored[name]
    for b in range(c["xs"].shape[0]):
        model, seen = host_class_loop(c, b)
        assert rel_err(out["models"][b], model.A) <= 1e-12 and rel_err(out["P"][b], model.P) <= 1e-12
        for h in range(out["hist"].shape[0]):
            assert rel_err(out["hist"][h, b], seen[5 * (h + 1) - 1], model.A) <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_two_experiments_are_the_same_snapshots(mirrored, name):
    """E = 2 experiments of N / 2 steps cut from the one trajectory: the same updates in the same order, bit for bit."""
    c, out = mirrored[name]
    two = online.online_dmdc_reference(**call_args(two_experiments(c), hist_every=5, innovations=True))
    for f in ("models", "P", "hist", "innov", "status"):
        assert np.array_equal(two[f], out[f]), f


# ---------------------------------------------------------------- the closed form
def closed_form(c, b, hermitian):
    """A_N = T_N M_N^-1, P_N = M_N^-1 with M_N = lam^N P0^-1 + sum_k lam^(N - k + 1) z_k z_k^T (z_k z_k^H), T_N likewise from
    A0 P0^-1 and y_k: no recursion, one inverse."""
    Z, Y = fit.stack_snapshots(c["xs"][b], c["us"], c["order"])
    nz, K = Z.shape
    lam = c["discount"]
    wgt = lam ** (K - np.arange(K))                   # lam^(N - k + 1), k = 1 .. N
    Zt = Z.conj() if hermitian else Z
    M = lam ** K * np.identity(nz) / c["alpha"] + (Z * wgt) @ Zt.T
    T = lam ** K * c["A0"] / c["alpha"] + (Y * wgt) @ Zt.T
    P = np.linalg.inv(M)
    return T @ P, P


@pytest.mark.parametrize("hermitian", [False, True], ids=["plain", "hermitian"])
@pytest.mark.parametrize("name", CASES)
def test_recursion_equals_the_closed_form(name, hermitian, record_property):
    """Measured where the bound was set: 8.5e-13 on A and 6.7e-13 on P at the worst; the bound is a hundred times that, because
    another draw moves it."""
    c = random_case(name, 11)
    out = online.online_dmdc_reference(**call_args(c, hermitian=hermitian))
    assert np.all(out["status"] == 0)
    worst = [0.0, 0.0]
    for b in range(c["xs"].shape[0]):
        A, P = closed_form(c, b, hermitian)
        worst = [max(worst[0], rel_err(out["models"][b], A)), max(worst[1], rel_err(out["P"][b], P))]
    record_property("rel_err_A", worst[0])
    record_property("rel_err_P", worst[1])
    print("case %s %s: A %.3g, P %.3g" % (name, "hermitian" if hermitian else "plain", *worst))
    assert worst[0] <= 1e-10 and worst[1] <= 1e-10


@pytest.mark.parametrize("name", ["a", "c"])
def test_hermitian_recursion_tends_to_the_least_squares_fit(name):
    """hermitian, discount = 1, A0 = 0, alpha = 1e8: P^-1 = G + 1e-8 I, so A is dmdc_fit_reference's full-rank fit (rcond = 1e-7)
    to 1e-6 - on data whose smallest singular value is above 1e-2 s_0 (asserted), so that nothing is truncated and the prior,
    1e-8 against lam_min >= 1e-4 lam_max, moves A by no more than 1e-8 / lam_min.  (Cases a and c: N >= nz, the data have full rank.)"""
    c = random_case(name, 12)
    n, nz = c["A0"].shape
    for b in range(c["xs"].shape[0]):
        s = np.linalg.svd(fit.stack_snapshots(c["xs"][b], c["us"], c["order"])[0], compute_uv=False)
        assert s[-1] > 1e-2 * s[0]
    out = online.online_dmdc_reference(c["xs"], c["us"], c["order"], np.zeros((n, nz)), alpha=1e8, discount=1.0, hermitian=True)
    want = fit.dmdc_fit_reference(c["xs"], c["us"], c["order"], 1e-7)
    assert np.all(want["rank"] == nz) and np.all(out["status"] == 0)
    assert rel_err(out["models"], want["models"]) <= 1e-6


# ---------------------------------------------------------------- counts, hist_every, innovations, non-finite data
def test_counts_hist_and_innovations_are_slices_of_a_plain_run(mirrored):
    c, full = mirrored["c"]
    c2 = two_experiments(c)                                   # [B, 2, 21, 9]
    full2 = online.online_dmdc_reference(**call_args(c2, innovations=True))
    counts = np.array([7, 0])
    out = online.online_dmdc_reference(**call_args(c2, counts=counts, hist_every=5, innovations=True))
    assert out["hist"].shape[0] == 8 and out["innov"].shape == (2, 40)
    # member 0: 7 steps of each experiment = a plain run on the truncated data
    cut = dict(c2, xs=np.ascontiguousarray(c2["xs"][:1, :, :8]), us=np.ascontiguousarray(c2["us"][:, :7]), u_scale=c2["u_scale"][:1])
    want = online.online_dmdc_reference(**call_args(cut, hist_every=5, innovations=True))
    assert np.array_equal(out["models"][0], want["models"][0]) and np.array_equal(out["P"][0], want["P"][0])
    assert want["hist"].shape[0] == 2 and np.array_equal(out["hist"][:2, 0], want["hist"][:, 0]) and not out["hist"][2:, 0].any()
    assert np.array_equal(out["innov"][0].reshape(2, 20)[:, :7], want["innov"][0].reshape(2, 7))
    assert not out["innov"][0].reshape(2, 20)[:, 7:].any()
    # the first experiment's innovations do not know what follows
    assert np.array_equal(out["innov"][0, :7], full2["innov"][0, :7])
    # member 1: no update at all
    assert np.array_equal(out["models"][1], c["A0"]) and np.array_equal(out["P"][1], ALPHA * np.identity(27))
    assert not out["hist"][:, 1].any() and not out["innov"][1].any() and list(out["status"]) == [0, 0]
    # hist_every and innovations change nothing else; the records are A after updates 5, 10, ...
    plain = online.online_dmdc_reference(**call_args(c))
    assert "innov" not in plain and plain["hist"].shape == (0, 2, 9, 27)
    assert np.array_equal(plain["models"], full["models"]) and np.array_equal(plain["P"], full["P"])
    first5 = online.online_dmdc_reference(**call_args(dict(c, xs=c["xs"][:, :, :6], us=c["us"][:5])))
    assert np.array_equal(full["hist"][0], first5["models"])
    # an innovation is |y - A z|^2 with the model BEFORE the update
    Z, Y = fit.stack_snapshots(c["xs"][0], c["u_scale"][0] * c["us"][None], c["order"])
    assert np.isclose(full["innov"][0, 0], np.linalg.norm(Y[:, 0] - c["A0"] @ Z[:, 0]) ** 2, rtol=1e-12)
    assert np.isclose(full["innov"][0, 5], np.linalg.norm(Y[:, 5] - full["hist"][0, 0] @ Z[:, 5]) ** 2, rtol=1e-9)


def test_per_member_arguments_equal_shared_ones(mirrored):
    c, full = mirrored["b"]
    B, nz = 2, 8
    out = online.online_dmdc_reference(c["xs"], np.broadcast_to(c["us"], (B, 1) + c["us"].shape), c["order"],
                                       np.broadcast_to(c["A0"], (B,) + c["A0"].shape), P0=np.broadcast_to(ALPHA * np.identity(nz), (B, nz, nz)),
                                       discount=np.full(B, c["discount"]), u_scale=c["u_scale"])
    assert np.array_equal(out["models"], full["models"]) and np.array_equal(out["P"], full["P"])


def test_a_member_with_nan_gets_status_3_and_zeros(mirrored):
    c, clean = mirrored["a"]
    xs = np.concatenate([c["xs"], c["xs"][:1]])
    u_scale = np.concatenate([c["u_scale"], c["u_scale"][:1]])
    xs[1, 0, 6, 2] = np.nan
    out = online.online_dmdc_reference(**call_args(c, xs=xs, u_scale=u_scale, hist_every=5, innovations=True))
    assert list(out["status"]) == [0, 3, 0]
    assert not out["models"][1].any() and not out["P"][1].any() and not out["hist"][:, 1].any()
    for b, src in ((0, 0), (2, 0)):
        assert np.array_equal(out["models"][b], clean["models"][src]) and np.array_equal(out["P"][b], clean["P"][src])
        assert np.array_equal(out["hist"][:, b], clean["hist"][:, src]) and np.array_equal(out["innov"][b], clean["innov"][src])
    # a non-finite sample beyond the member's count is never taken
    late = online.online_dmdc_reference(**call_args(c, xs=xs, u_scale=u_scale, counts=np.array([12, 5, 12])))
    assert list(late["status"]) == [0, 0, 0]
    us = np.broadcast_to(c["us"], (3, 1) + c["us"].shape).copy()
    us[2, 0, 3, 0] = np.inf
    assert list(online.online_dmdc_reference(**call_args(c, xs=np.concatenate([c["xs"], c["xs"][:1]]), us=us,
                                                         u_scale=u_scale))["status"]) == [0, 0, 3]


# ---------------------------------------------------------------- the Python layer
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _args(B=3, E=2, N=4, n=9, m=2):
    return dict(xs=np.zeros((B, E, N + 1, n), complex), us=np.zeros((E, N, m)), order=1, A0=np.zeros((n, 3 * n)), alpha=1e2)


ONLINE_BAD = [dict(xs=np.zeros((3, 9))), dict(xs=np.zeros((3, 2, 1, 9))), dict(us=np.zeros((2, 5, 2))), dict(order=0),
              dict(u_scale=np.ones((2, 2))), dict(A0=np.zeros((9, 26))), dict(A0=np.zeros((2, 9, 27))), dict(A0=np.zeros((3, 27, 9))),
              dict(alpha=None), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha=float("inf")),
              dict(alpha=np.ones(3)), dict(P0=np.identity(27)), dict(alpha=None, P0=np.identity(26)),
              dict(alpha=None, P0=np.zeros((2, 27, 27))), dict(discount=0.0), dict(discount=1.0001), dict(discount=-0.5),
              dict(discount=float("nan")), dict(discount=np.full(2, 0.9)), dict(discount=np.array([0.9, 0.9, 1.5])),
              dict(counts=np.array([1, 2])), dict(counts=np.array([1, 2, 5])), dict(counts=np.array([1, -1, 2])),
              dict(counts=np.array([1.0, 2.0, 3.0])), dict(hist_every=-1), dict(hist_every=2.5), dict(hist_every=True)]


@pytest.mark.parametrize("change", ONLINE_BAD, ids=lambda c: ",".join("%s=%s" % (k, getattr(v, "shape", v)) for k, v in c.items()))
def test_online_calls_refuse_malformed_arguments(no_library, change):
    args = dict(_args(), **change)
    with pytest.raises(ValueError):
        m4q.online_dmdc_batch(**args)
    with pytest.raises(ValueError):
        m4q.online_dmdc_reference(**args)


def test_wrapper_hands_the_kernel_what_it_was_given(monkeypatch):
    seen = {}

    class Fake:
        def m4q_online_dmdc_batch(self, *a):
            seen["a"] = a
            return 0

        def m4q_last_error(self):
            return b""
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    B, E, N, n, m = 3, 2, 4, 9, 2
    out = m4q.online_dmdc_batch(np.zeros((B, E, N + 1, n)), np.zeros((E, N, m)), 1, np.zeros((n, 27)), alpha=50.0, discount=0.9,
                                u_scale=np.ones((B, m)), counts=[4, 0, 2], hermitian=True, hist_every=3, innovations=True)
    a = seen["a"]
    assert a[:6] == (B, n, m, 1, E, N) and a[8] == 0 and a[9] is not None and a[12] == 0 and a[13] is None and a[14] == 0
    assert a[15] == 50.0 and a[17] == 0 and a[18] == _lib.ONLINE_HERMITIAN and a[19] == 3
    assert list(np.ctypeslib.as_array(a[10], (B,))) == [4, 0, 2] and np.ctypeslib.as_array(a[16], (1,))[0] == 0.9
    assert out["models"].shape == (B, n, 27) and out["P"].shape == (B, 27, 27) and out["hist"].shape == (2, B, n, 27)
    assert out["innov"].shape == (B, 8) and out["status"].shape == (B,)
    out = m4q.online_dmdc_batch(np.zeros((B, N + 1, n)), np.zeros((B, N, m)), 1, np.zeros((B, n, 27)), P0=np.zeros((B, 27, 27)),
                                discount=np.full(B, 0.9))
    a = seen["a"]
    assert a[:6] == (B, n, m, 1, 1, N) and a[8] == 1 and a[9] is None and a[10] is None and a[12] == 1 and a[13] is not None
    assert a[14] == 1 and a[17] == 1 and a[18] == 0 and a[19] == 0 and a[22] is None and a[23] is None
    assert out["hist"].shape == (0, B, n, 27) and "innov" not in out


def test_prototype_and_exports():
    assert len(_lib.PROTOTYPES["m4q_online_dmdc_batch"][1]) == 25
    assert m4q.online_dmdc_batch is online.online_dmdc_batch and m4q.online_dmdc_reference is online.online_dmdc_reference
    assert m4q.stream_models_batch is online.stream_models_batch


def test_from_batch_continues_on_the_host(mirrored):
    """The first 7 updates in the batch form, the rest through fit_iteration on the object from_batch returns."""
    c, full = mirrored["b"]
    part = online.online_dmdc_reference(**call_args(c, counts=np.array([7, 7])))
    for b in range(2):
        model = m4q.OnlineDMDc.from_batch(part, b)
        assert isinstance(model, m4q.OnlineDMDc) and (model.dim_y, model.dim_x, model.dim_u) == (4, 4, 4)
        model.discount = c["discount"]
        Z, Y = fit.stack_snapshots(c["xs"][b], c["u_scale"][b] * c["us"][None], c["order"])
        for k in range(7, 12):
            model.fit_iteration(Y[:, k], Z[:4, k], Z[4:, k])
        assert rel_err(model.A, full["models"][b]) <= 1e-12 and rel_err(model.P, full["P"][b]) <= 1e-12
        assert model.get_discrete()[0].shape == (4, 4)


# ---------------------------------------------------------------- streaming for an ensemble
class _Clock:
    def __init__(self, measure_freq):
        self.measure_freq = measure_freq


def _fake_run(rng, B=3, n=4, m=1, ns=9):
    xs = rng.standard_normal((B, ns + 1, n)) + 1j * rng.standard_normal((B, ns + 1, n))
    xs /= np.linalg.norm(xs, axis=-1, keepdims=True)
    return {"xs": xs, "us": rng.uniform(-1, 1, (B, ns, m)), "steps_done": np.array([ns, 4, 0], dtype=np.int32),
            "exit_codes": np.array([0, 1, 1], dtype=np.int32)}


def test_streaming_helper_equals_the_class_fed_by_hand():
    """A fake run dict in both layouts (a session's results(): time axis second; mpc_batch: last), a member that ended early and
    one that never stepped: the helper is OnlineDMDc fed with the steps the run kept, as mpc(streaming=True) feeds it."""
    rng = np.random.default_rng(21)
    run = _fake_run(rng)
    B, n, nz = 3, 4, 8
    models = 0.1 * (rng.standard_normal((B, n, nz)) + 1j * rng.standard_normal((B, n, nz)))
    got = m4q.stream_models_batch(run, models, 1, _Clock(1), alpha=ALPHA, discount=0.97, reference=True)
    swapped = dict(run, xs=np.swapaxes(run["xs"], 1, 2), us=np.swapaxes(run["us"], 1, 2))
    same = m4q.stream_models_batch(swapped, models, 1, _Clock(1), alpha=ALPHA, discount=0.97, reference=True)
    assert np.array_equal(got["models"], same["models"]) and np.array_equal(got["P"], same["P"])
    wrap = m4q.WrapModel(models[0][:, :n], models[0][:, n:], 1, 1)
    for b in range(B):
        model = m4q.OnlineDMDc.from_bootstrap(n, n, nz - n, models[b].copy(), alpha=ALPHA)
        model.discount = 0.97
        for step in range(run["steps_done"][b]):
            lx = run["xs"][b, step].reshape(-1, 1)
            lu = wrap.lift_u(run["us"][b, step].reshape(-1, 1))
            model.fit_iteration(run["xs"][b, step + 1].reshape(-1, 1), lx, m4q.krtimes(lu, lx))          # mpc.py:281-285
        assert rel_err(got["models"][b], model.A) <= 1e-12 and rel_err(got["P"][b], model.P) <= 1e-12
    assert np.array_equal(got["models"][2], models[2])
    shared = m4q.stream_models_batch(run, models[0], 1, _Clock(1), alpha=ALPHA, reference=True)
    assert shared["models"].shape == (B, n, nz)


def test_streaming_helper_refusals(no_library):
    rng = np.random.default_rng(22)
    run = _fake_run(rng)
    models = np.zeros((3, 4, 8), complex)
    with pytest.raises(ValueError, match="measure_freq"):
        m4q.stream_models_batch(run, models, 1, _Clock(2), alpha=ALPHA)
    with pytest.raises(ValueError):
        m4q.stream_models_batch(run, models, 1, _Clock(1))                                    # neither alpha nor P0
    with pytest.raises(ValueError):
        m4q.stream_models_batch(run, np.zeros((3, 5, 10), complex), 1, _Clock(1), alpha=ALPHA)   # models of another n
    with pytest.raises(ValueError):
        m4q.stream_models_batch(run, models, 1, _Clock(1), alpha=ALPHA, layout="sideways")
    square = {"xs": np.zeros((3, 4, 4), complex), "us": np.zeros((3, 3, 3)), "steps_done": np.zeros(3, np.int32)}
    with pytest.raises(ValueError, match="time axis"):
        m4q.stream_models_batch(square, np.zeros((4, 16), complex), 1, _Clock(1), alpha=ALPHA)


# ---------------------------------------------------------------- the C ABI
class _OnlineCall:
    """One valid m4q_online_dmdc_batch call on host buffers of the right sizes; fields are replaced one at a time."""

    def __init__(self, B=3, n=9, m=2, order=1, E=2, N=4, P=2):
        nz = n * (1 + P)
        self.keep = {}
        self.v = dict(B=B, n=n, m=m, order=order, E=E, N=N, xs=self._b("xs", 2 * B * E * (N + 1) * n), u=self._b("u", E * N * m), u_per=0,
                      u_scale=None, counts=None, A0=self._b("A0", 2 * n * nz), A0_per=0, P0=None, P0_per=0, alpha=1e2,
                      discount=self._b("discount", B, 0.97), discount_per=0, flags=0, hist_every=0,
                      models=self._b("models", 2 * B * n * nz), P=self._b("P", 2 * B * nz * nz), hist=self._b("hist", 2 * E * N * B * n * nz),
                      innov=self._b("innov", B * E * N), status=self._i("status", B))

    def _b(self, name, count, fill=0.0):
        self.keep[name] = np.full(max(int(count), 1), fill, dtype=np.float64)
        return self.keep[name].ctypes.data_as(DP)

    def _i(self, name, count):
        self.keep[name] = np.zeros(max(int(count), 1), dtype=np.int32)
        return self.keep[name].ctypes.data_as(IP)

    def __call__(self, value=None, counts=None, **change):
        """value: the discount (of member 1 when discount_per is set); discount=None in `change` is the missing pointer."""
        v = dict(self.v, **change)
        if value is not None:
            self.keep["discount"][:] = 0.97
            self.keep["discount"][min(1, v["B"] - 1) if v["discount_per"] else 0] = value
        if counts is not None:
            v["counts"] = self._i("counts", len(counts))
            self.keep["counts"][:] = counts
        order = ("B", "n", "m", "order", "E", "N", "xs", "u", "u_per", "u_scale", "counts", "A0", "A0_per", "P0", "P0_per", "alpha",
                 "discount", "discount_per", "flags", "hist_every", "models", "P", "hist", "innov", "status")
        return _lib.lib().m4q_online_dmdc_batch(*[v[k] for k in order])


@pytest.mark.parametrize("change", [dict(B=0), dict(B=-1), dict(E=0), dict(E=-3), dict(N=0), dict(N=-1), dict(hist_every=-1),
                                    dict(flags=2), dict(flags=-1), dict(xs=None), dict(u=None), dict(A0=None), dict(discount=None),
                                    dict(models=None), dict(status=None), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("nan")),
                                    dict(alpha=float("inf")), dict(value=0.0), dict(value=-0.5), dict(value=1.0000001),
                                    dict(value=float("nan")), dict(value=float("inf")), dict(value=2.0, discount_per=1),
                                    dict(counts=[1, 5, 2]), dict(counts=[-1, 0, 0]), dict(counts=[0, 0, 1 << 30])], ids=str)
def test_online_refuses_bad_arguments(change):
    assert _OnlineCall()(**change) == _lib.E_BADARG
    assert _lib.lib().m4q_last_error()


def test_online_refuses_shapes_without_a_kernel():
    assert _OnlineCall(n=25)() == _lib.E_UNSUPPORTED                              # no compiled shape
    assert _OnlineCall(n=9, order=3, P=9)() == _lib.E_UNSUPPORTED
    assert _OnlineCall(n=16, m=2, order=1, P=2)() == _lib.E_UNSUPPORTED           # the plant-only shape has no model
    assert _OnlineCall(n=16, m=1, order=4, P=4)() == _lib.E_UNSUPPORTED           # nz = 80: more than one lane per wavefront's 64
    assert b"nz = 80" in _lib.lib().m4q_last_error()


def test_valid_online_calls_need_a_device():
    """The range ends, the optional arguments left out or given and every supported shape get as far as asking for a device."""
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    call = _OnlineCall()
    assert call() == _lib.E_NODEVICE
    assert call(value=1.0) == _lib.E_NODEVICE and call(value=1e-300) == _lib.E_NODEVICE
    assert call(value=0.5, discount_per=1) == _lib.E_NODEVICE
    assert call(counts=[0, 4, 2]) == _lib.E_NODEVICE
    assert call(flags=_lib.ONLINE_HERMITIAN, hist_every=3) == _lib.E_NODEVICE
    assert call(P=None, hist=None, innov=None) == _lib.E_NODEVICE
    assert call(alpha=0.0, P0=call._b("P0", 2 * 27 * 27)) == _lib.E_NODEVICE      # an explicit P0 needs no alpha
    for n, m, order, P in ((4, 1, 1, 1), (4, 1, 2, 2), (4, 2, 1, 2), (9, 2, 2, 5), (16, 3, 1, 3), (16, 1, 1, 1), (16, 1, 2, 2),
                           (16, 1, 3, 3), (8, 2, 1, 2)):
        assert _OnlineCall(n=n, m=m, order=order, P=P)() == _lib.E_NODEVICE, (n, m, order)
    with pytest.raises(_lib.M4qError):
        m4q.online_dmdc_batch(np.zeros((2, 5, 4)), np.zeros((4, 1)), 1, np.zeros((4, 8)), alpha=1e2)

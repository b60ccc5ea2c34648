"""CPU checks of the feedback runs (m4q_plant_feedback_batch, m4q_model_feedback_batch; mpc4quantum_amd/feedback.py): the NumPy
definition against an independent closed loop of a few lines, the law's formula at its corners, every refusal of the C ABI with its
code before a device is asked for, the Python wrappers' refusals before the library is touched, and what the wrapper hands the
kernel."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, feedback
from tests import feedback_cases as fc
from tests import grad_cases as gc

DP, IP = _lib._dp, _lib._ip


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("name", fc.PLANTS)
def test_definition_against_an_independent_loop(name):
    """Per-member law, u_scale, per-member operators, a non-uniform grid, the band: the definition's states, controls and counts
    against the loop written out with the oracle's plant step and np.clip.  Both loops take the same decisions unless some s_k
    lies within rounding of a bound; the seeds keep every s_k 1e-9 away."""
    c = fc.case(name)
    B, N = 3, 6
    rng = np.random.default_rng(9000 + fc.PLANTS.index(name))
    x0 = c.states(rng, B)
    op0, ops = c.member_ops(rng, B)
    if c.exp is not None:
        ops = np.stack([c.ops] * B)
    ts = fc._grid(rng, N, c.dt)
    sc = 1 + 0.1 * rng.standard_normal((B, c.m))
    law = fc.make_law(rng, c.n, c.m, N, c.sat, x0[0], members=B)
    W, f = gc.weights_and_targets(rng, c.n, B)
    got = m4q.plant_feedback_reference(x0, law, op0, ops, ts, c.kind, u_scale=sc, W=W, target=f, figure="all")
    xs, us, clipped = fc.independent_plant_run(c, x0, law, op0, ops, np.diff(ts), sc)
    _, s, lo, hi, _ = fc.law_terms(law, got["xs"], got["us"])
    assert min(np.abs(s - lo).min(), np.abs(s - hi).min()) > 1e-9
    assert np.abs(got["us"] - us).max() <= 1e-10 * c.sat
    assert np.abs(got["xs"] - xs).max() <= 1e-10 * max(1.0, np.abs(xs).max())
    assert np.array_equal(got["clipped"], clipped) and got["clipped"].dtype == np.int32 and clipped.min() > 0
    assert np.array_equal(got["status"], np.zeros(B, np.int32))
    assert np.array_equal(got["xs"][:, 0].view(np.float64), x0.view(np.float64))
    q = fc.figures(xs, W, f)
    assert np.abs(got["q"] - q).max() <= 1e-10 * max(1.0, np.abs(q).max())
    last = m4q.plant_feedback_reference(x0, law, op0, ops, ts, c.kind, u_scale=sc, W=W, target=f, keep="last", figure="last")
    assert np.array_equal(last["xs"], got["xs"][:, N]) and np.array_equal(last["q"], got["q"][:, N])
    assert set(m4q.plant_feedback_reference(x0, law, op0, ops, ts, c.kind, keep="none")) == {"us", "clipped", "status"}


@pytest.mark.parametrize("shape", [(4, 1, 2), (9, 2, 2), (8, 2, 1)], ids=lambda s: "%d-%d-%d" % s)
def test_model_definition_against_the_oracle_model(shape):
    n, m, order = shape
    B, N = 3, 5
    models, x0, sat, rng = gc.model_case(n, m, order, B, 9100 + n)
    law = fc.make_law(rng, n, m, N, sat, x0[0])
    sc = 1 + 0.1 * rng.standard_normal((B, m))
    got = m4q.model_feedback_reference(x0, law, models, order, u_scale=sc)
    for b in range(B):
        chain = gc.model_chain(models[b], m, order, x0[b], sc[b] * got["us"][b])
        assert np.abs(got["xs"][b] - chain).max() <= 1e-10 * max(1.0, np.abs(chain).max())
    u, s, lo, hi, _ = fc.law_terms(law, got["xs"], got["us"])
    assert np.array_equal(u, got["us"])
    assert np.array_equal(got["clipped"], ((s <= lo) | (s >= hi)).sum(axis=(1, 2)))


def test_control_band_box_and_their_order():
    n, m, N = 4, 2, 2
    K = np.zeros((N, n + 1, m), complex)
    K[0, 1, 0], K[0, 4, 0], K[0, 2, 1] = 2.0 - 1.0j, 0.25 + 9.0j, 1.0j          # (the affine column's imaginary part is not read)
    x_ref = np.zeros((N + 1, n), complex)
    x_ref[0, 1] = 0.5
    u_ref = np.array([[0.1, -0.2], [0.0, 0.0]])
    x = np.array([0, 1.5 + 0.5j, 2.0 - 3.0j, 0])
    s = np.array([2.0 * 1.0 + 1.0 * 0.5 + 0.25 + 0.1, 3.0 - 0.2])                # Re(K d): (2 - i)(1 + 0.5 i) -> 2.5; i (2 - 3 i) -> 3
    free = m4q.FeedbackLaw(K, x_ref, u_ref, np.inf)
    u, s_, lo, hi = free.terms(0, x)
    assert np.allclose(s_, s, rtol=0, atol=1e-15) and np.array_equal(u, s_) and np.all(lo == -np.inf) and np.all(hi == np.inf)
    assert np.array_equal(free.control(0, x), u)
    box = m4q.FeedbackLaw(K, x_ref[:N], u_ref, 2.82)
    assert np.allclose(box.control(0, x), [2.82, 2.8], rtol=0, atol=1e-15)
    band = m4q.FeedbackLaw(K, x_ref, u_ref, 2.9, du=0.5, u_prev=[2.0, -1.0])
    u, _, lo, hi = band.terms(0, x)
    assert np.array_equal(lo, [1.5, -1.5]) and np.array_equal(hi, [2.5, -0.5]) and np.array_equal(u, [2.5, -0.5])
    assert np.allclose(band.control(0, x, p=[3.0, 4.0]), [2.85, 2.9], rtol=0, atol=1e-15)     # lo = 3.5 > hi = 2.9: hi, the box, wins
    assert np.array_equal(band.control(1, x, p=[5.0, -5.0]), [2.9, -4.5])        # lo = 4.5 > hi = 2.9: hi wins; lo = -2.9 > hi = -4.5: hi wins
    per = m4q.FeedbackLaw(np.stack([K, 2 * K]), np.stack([x_ref, x_ref]), np.stack([u_ref, u_ref]), np.inf)
    assert per.members == 2 and np.allclose(per.control(0, x, member=1), 2 * s - u_ref[0], rtol=0, atol=1e-14)
    nan = box.control(0, np.full(n, np.nan))
    assert np.array_equal(nan, [-2.82, -2.82])                                     # fmin(fmax(NaN, lo), hi) = lo, as on the device


@pytest.mark.parametrize("bad", [dict(gains=np.zeros((2, 5))), dict(x_ref=np.zeros((4, 4))), dict(x_ref=np.zeros((2, 3))),
                                 dict(u_ref=np.zeros((3, 2))), dict(u_ref=np.zeros((1, 2, 2))), dict(sat=0.0), dict(sat=-1.0),
                                 dict(sat=np.nan), dict(du=0.0), dict(du=np.inf), dict(du=-0.1), dict(du=0.1),
                                 dict(du=0.1, u_prev=np.zeros(3)), dict(u_prev=np.zeros((2, 2, 2))),
                                 dict(gains=np.zeros((3, 2, 5, 2)))], ids=str)
def test_law_refuses_bad_shapes_and_values(bad):
    args = dict(gains=np.zeros((2, 5, 2), complex), x_ref=np.zeros((3, 4), complex), u_ref=np.zeros((2, 2)), sat=1.0)
    with pytest.raises(ValueError):
        m4q.FeedbackLaw(**dict(args, **bad))
    with pytest.raises(TypeError):
        m4q.FeedbackLaw(**dict(args, u_ref=np.zeros((2, 2), complex)))


@pytest.mark.parametrize("kind", ["iid", "hermitian"])
def test_noisy_definition_leaves_the_noise_as_its_residual(kind):
    c = fc.case("9-2-hamiltonian")
    B, N = 3, 4
    rng = np.random.default_rng(9200)
    x0 = c.states(rng, B)
    law = fc.make_law(rng, c.n, c.m, N, c.sat, x0[0])
    noise = m4q.MeasurementNoise(np.array([0.0, 0.02, 0.05]), 77, kind, member_base=1 << 33)
    got = m4q.plant_feedback_reference(x0, law, c.op0, c.ops, c.dt, c.kind, noise=noise)
    free = m4q.plant_feedback_reference(x0, law, c.op0, c.ops, c.dt, c.kind)
    res = fc.step_residuals(lambda b, t, x, v: c.step(x, v, c.op0, list(c.ops), c.dt), got["xs"], got["us"], np.ones((B, c.m)))
    for t in range(N):
        assert np.abs(res[:, t] - noise.sample(np.arange(B), t + 1, c.n)).max() <= 1e-12
    assert np.array_equal(got["xs"][0], free["xs"][0]) and np.abs(got["xs"][2] - free["xs"][2]).max() > 1e-3
    u, _, _, _, _ = fc.law_terms(law, got["xs"], got["us"])
    assert np.array_equal(u, got["us"])                                          # the next control sees the noisy state
    assert np.array_equal(got["xs"][:, 0], x0)                                   # x0 is never measured


def test_status_and_clipped_of_a_lost_member():
    c = fc.case("4-1-hamiltonian")
    B, N = 3, 4
    rng = np.random.default_rng(9300)
    x0 = c.states(rng, B)
    law = fc.make_law(rng, c.n, c.m, N, c.sat, x0[0])
    good = m4q.plant_feedback_reference(x0, law, c.op0, c.ops, c.dt, c.kind)
    x0[1, 2] = np.nan
    got = m4q.plant_feedback_reference(x0, law, c.op0, c.ops, c.dt, c.kind)
    assert np.array_equal(got["status"], [0, 3, 0]) and got["status"].dtype == np.int32
    assert got["clipped"][1] == 0                                                # a NaN s_k is at neither bound
    for b in (0, 2):
        assert np.array_equal(got["xs"][b], good["xs"][b]) and got["clipped"][b] == good["clipped"][b]
    free = m4q.FeedbackLaw(law.gains, law.x_ref, law.u_ref, np.inf)
    with np.errstate(invalid="ignore"):                                          # (its controls are -inf: inf * 0 in the plant step)
        assert m4q.plant_feedback_reference(x0, free, c.op0, c.ops, c.dt, c.kind)["status"][1] == 3


def test_from_quad_program_shapes():
    g = np.zeros((3, 4, 5, 2), complex)
    X, U = np.zeros((1, 5, 4), complex), np.zeros((1, 4, 2))
    law = m4q.FeedbackLaw.from_quad_program(g, X, U, 1.0)
    assert law.members == 3 and law.x_ref.shape == (3, 4, 4) and law.u_ref.shape == (3, 4, 2) and law.N == 4
    law = m4q.FeedbackLaw.from_quad_program(g[0], X, U[0], 1.0)
    assert law.members is None and law.x_ref.shape == (4, 4)
    law = m4q.FeedbackLaw.from_quad_program(g, np.zeros((3, 5, 4)), np.zeros((3, 4, 2)), 2.0, du=0.5, u_prev=np.zeros((3, 2)))
    assert law.prev_members == 3 and law.du == 0.5


# ---------------------------------------------------------------- the C ABI
def _buf(n, dtype=np.float64):
    a = np.zeros(max(int(n), 1), dtype=dtype)
    return a, a.ctypes.data_as(IP if dtype == np.int32 else DP)


class _Call:
    def _b(self, name, count, dtype=np.float64):
        self.keep[name], p = _buf(count, dtype)
        return p

    def _shared(self, B, n, m, N):
        sigma, sp = _buf(1)
        sigma[0] = 0.1
        self.keep["sigma"] = sigma
        return dict(B=B, n=n, m=m, N=N, x0=self._b("x0", 2 * B * n), gains=self._b("g", 2 * N * (n + 1) * m), x_ref=self._b("xr", 2 * N * n),
                    u_ref=self._b("ur", N * m), law_per=0, sat=1.0, band=0, du=0.0, u_prev=self._b("up", m), up_per=0, u_scale=None,
                    noise=0, sigma=sp, s_per=0, seed=5, base=0, W=self._b("W", 2 * n * n), target=self._b("f", 2 * n), t_per=0,
                    xs_mode=2, xs=self._b("xs", 2 * B * (N + 1) * n), q_mode=2, q=self._b("q", B * (N + 1)), us=self._b("us", B * N * m),
                    clipped=self._b("cl", B, np.int32), status=self._b("st", B, np.int32))

    def _tail(self, v):
        return (v["noise"], v["sigma"], v["s_per"], v["seed"], v["base"], v["W"], v["target"], v["t_per"], v["xs_mode"], v["xs"],
                v["q_mode"], v["q"], v["us"], v["clipped"], v["status"])

    def _law(self, v):
        return (v["gains"], v["x_ref"], v["u_ref"], v["law_per"], v["sat"], v["band"], v["du"], v["u_prev"], v["up_per"], v["u_scale"])


class _PlantCall(_Call):
    """One valid m4q_plant_feedback_batch call on host buffers of the right sizes; fields are replaced one at a time."""

    def __init__(self, B=3, n=9, m=2, kind=_lib.PLANT_HAMILTONIAN, N=4, k=3):
        self.keep = {}
        self.v = dict(self._shared(B, n, m, N), kind=kind, dts=self._b("dts", N), op0=self._b("op0", 2 * k * k),
                      ops=self._b("ops", 2 * m * k * k), per=0)

    def __call__(self, **change):
        v = dict(self.v, **change)
        return _lib.lib().m4q_plant_feedback_batch(v["B"], v["n"], v["m"], v["kind"], v["N"], v["dts"], v["x0"], *self._law(v), v["op0"],
                                                   v["ops"], v["per"], *self._tail(v))


class _ModelCall(_Call):
    def __init__(self, B=3, n=9, m=2, order=1, N=4, P=2):
        self.keep = {}
        self.v = dict(self._shared(B, n, m, N), order=order, models=self._b("models", 2 * n * n * (1 + P)), m_per=0)

    def __call__(self, **change):
        v = dict(self.v, **change)
        return _lib.lib().m4q_model_feedback_batch(v["B"], v["n"], v["m"], v["order"], v["N"], v["x0"], *self._law(v), v["models"],
                                                   v["m_per"], *self._tail(v))


BAD_COMMON = [dict(B=0), dict(B=-2), dict(N=0), dict(N=-1), dict(x0=None), dict(gains=None), dict(x_ref=None), dict(u_ref=None),
              dict(status=None), dict(sat=0.0), dict(sat=-1.0), dict(sat=float("nan")), dict(band=1, du=0.0), dict(band=1, du=-0.5),
              dict(band=1, du=float("inf")), dict(band=1, du=float("nan")), dict(band=1, du=0.5, u_prev=None),
              dict(xs_mode=3), dict(xs_mode=-1), dict(q_mode=3), dict(q_mode=-1),
              dict(xs_mode=0, q_mode=0, us=None, clipped=None), dict(xs=None), dict(q=None), dict(W=None), dict(target=None),
              dict(q_mode=1, W=None), dict(q_mode=1, target=None), dict(noise=3), dict(noise=-1), dict(noise=1, sigma=None),
              dict(noise=2, sigma=None)]


@pytest.mark.parametrize("change", BAD_COMMON + [dict(dts=None), dict(op0=None), dict(ops=None), dict(kind=0), dict(kind=4),
                                                 dict(kind=-1), dict(kind=_lib.PLANT_PROCESS)], ids=str)
def test_plant_feedback_refuses_bad_arguments(change):
    """(kind = PROCESS on n = 9: not a fourth power.)"""
    assert _PlantCall()(**change) == _lib.E_BADARG
    assert _lib.lib().m4q_last_error()


@pytest.mark.parametrize("change", BAD_COMMON + [dict(models=None)], ids=str)
def test_model_feedback_refuses_bad_arguments(change):
    assert _ModelCall()(**change) == _lib.E_BADARG
    assert _lib.lib().m4q_last_error()


def test_hermitian_noise_needs_a_density_matrix():
    assert _PlantCall(n=16, m=1, kind=_lib.PLANT_PROCESS, k=2)(noise=_lib.NOISE_HERMITIAN) == _lib.E_BADARG
    assert _ModelCall(n=8, m=2)(noise=_lib.NOISE_HERMITIAN) == _lib.E_BADARG
    call = _PlantCall()
    call.keep["sigma"][0] = -0.1
    assert call(noise=_lib.NOISE_IID) == _lib.E_BADARG                          # a negative sigma


def test_feedback_refuses_shapes_without_a_kernel():
    assert _PlantCall(n=25, k=5)() == _lib.E_UNSUPPORTED                       # no compiled shape
    assert _PlantCall(n=9, m=3)() == _lib.E_UNSUPPORTED
    assert _PlantCall(n=8, m=2, k=2)() == _lib.E_UNSUPPORTED                   # a shape with a model and no device plant
    assert _ModelCall(n=25, P=2)() == _lib.E_UNSUPPORTED
    assert _ModelCall(n=9, order=3, P=9)() == _lib.E_UNSUPPORTED
    assert _ModelCall(n=16, m=2, order=1, P=2)() == _lib.E_UNSUPPORTED         # the plant-only shape has no model kernel


def test_valid_calls_need_a_device():
    """Every optional output through NULL, every noise kind where it is allowed, all three plants, the plant-only shape."""
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    for call in (_PlantCall(), _PlantCall(n=16, m=2, k=4), _PlantCall(n=16, m=1, kind=_lib.PLANT_PROCESS, k=2),
                 _PlantCall(n=9, kind=_lib.PLANT_GENERATOR, k=9), _ModelCall(), _ModelCall(n=8, m=2), _ModelCall(n=16, m=1, order=4, P=4)):
        assert call() == _lib.E_NODEVICE
        assert call(noise=_lib.NOISE_IID) == _lib.E_NODEVICE
        assert call(band=1, du=0.5) == _lib.E_NODEVICE
        assert call(q_mode=0, W=None, target=None, q=None) == _lib.E_NODEVICE
        assert call(xs_mode=0, xs=None, us=None) == _lib.E_NODEVICE
        assert call(xs_mode=0, xs=None, q_mode=0, q=None, W=None, target=None, us=None) == _lib.E_NODEVICE     # clipped alone
        assert call(clipped=None, u_prev=None, sigma=None, sat=float("inf")) == _lib.E_NODEVICE
    assert _PlantCall()(noise=_lib.NOISE_HERMITIAN) == _lib.E_NODEVICE
    assert _PlantCall(n=9, kind=_lib.PLANT_GENERATOR, k=9)(noise=_lib.NOISE_HERMITIAN) == _lib.E_NODEVICE
    assert _ModelCall()(noise=_lib.NOISE_HERMITIAN) == _lib.E_NODEVICE
    law = m4q.FeedbackLaw(np.zeros((3, 5, 1)), np.zeros((3, 4)), np.zeros((3, 1)), 1.0)
    with pytest.raises(_lib.M4qError):
        m4q.plant_feedback_batch(np.zeros((1, 4)), law, np.eye(2), np.eye(2)[None], 0.1)
    with pytest.raises(_lib.M4qError):
        m4q.model_feedback_batch(np.zeros((1, 4)), law, np.zeros((4, 8)), 1)


# ---------------------------------------------------------------- the Python wrappers
@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library is a failure: shapes are refused before it is loaded."""
    def boom():
        raise AssertionError("the library was touched before the shapes were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _law(N=4, n=9, m=2, members=None, **kw):
    lead = () if members is None else (members,)
    return m4q.FeedbackLaw(np.zeros(lead + (N, n + 1, m)), np.zeros(lead + (N, n)), np.zeros(lead + (N, m)), 1.0, **kw)


def _plant_args(B=3, n=9, m=2, N=4, k=3):
    return dict(x0=np.zeros((B, n), complex), law=_law(N, n, m), op0=np.zeros((k, k), complex), ops=np.zeros((m, k, k), complex),
                dt_or_ts=0.25)


PLANT_BAD = [dict(x0=np.zeros(9)), dict(x0=np.zeros((3, 4))), dict(x0=np.zeros((0, 9))), dict(law=_law(members=2)),
             dict(law=_law(m=1)), dict(law=_law(du=0.1, u_prev=np.zeros((2, 2)))), dict(op0=np.zeros((2, 2))),
             dict(ops=np.zeros((1, 3, 3))), dict(dt_or_ts=np.zeros(4)), dict(dt_or_ts=np.inf), dict(u_scale=np.ones((3, 1))),
             dict(kind=0), dict(kind=7), dict(kind=_lib.PLANT_PROCESS), dict(kind=_lib.PLANT_GENERATOR), dict(keep="first"),
             dict(figure="sum"), dict(figure="all"), dict(figure="last", W=np.eye(9)), dict(figure="all", W=np.eye(4), target=np.zeros(9)),
             dict(noise=m4q.MeasurementNoise(np.ones(2), 1)), dict(noise=m4q.MeasurementNoise(0.1, 1, member_base=(1 << 64) - 1))]


@pytest.mark.parametrize("change", PLANT_BAD, ids=lambda c: ",".join("%s%s" % (k, getattr(v, "shape", "")) for k, v in c.items()))
def test_plant_feedback_wrapper_refuses_bad_arguments(no_library, change):
    with pytest.raises(ValueError):
        m4q.plant_feedback_batch(**dict(_plant_args(), **change))
    with pytest.raises(ValueError):
        m4q.plant_feedback_reference(**dict(_plant_args(), **change))


def test_wrappers_refuse_wrong_types_and_noise_kinds(no_library):
    with pytest.raises(TypeError):
        m4q.plant_feedback_batch(**dict(_plant_args(), law=np.zeros((4, 10, 2))))
    with pytest.raises(TypeError):
        m4q.plant_feedback_batch(**dict(_plant_args(), noise=0.1))
    with pytest.raises(TypeError):
        m4q.model_feedback_batch(np.zeros((3, 9)), None, np.zeros((9, 27)), 1)
    herm = m4q.MeasurementNoise(0.1, 1, "hermitian")
    with pytest.raises(ValueError):                                              # a process vector is no density matrix
        m4q.plant_feedback_batch(np.zeros((3, 16)), _law(n=16, m=1), np.zeros((2, 2)), np.zeros((1, 2, 2)), 0.1, _lib.PLANT_PROCESS,
                                 noise=herm)
    with pytest.raises(ValueError):                                              # n = 8 is no square
        m4q.model_feedback_batch(np.zeros((3, 8)), _law(n=8), np.zeros((8, 24)), 1, noise=herm)
    args = dict(x0=np.zeros((3, 9), complex), law=_law(), models=np.zeros((9, 27), complex), order=1)
    for change in (dict(x0=np.zeros(9)), dict(models=np.zeros((9, 18))), dict(models=np.zeros((2, 9, 27))), dict(order=2), dict(order=0),
                   dict(law=_law(n=4)), dict(u_scale=np.ones((3, 3))), dict(figure="last"), dict(keep="every")):
        with pytest.raises(ValueError):
            m4q.model_feedback_batch(**dict(args, **change))
    H0, Hk = np.diag([0.0, 1.0, 2.0]), [np.eye(3), np.eye(3)]
    ts = np.arange(5) * 0.25
    for exp in (m4q.QExperiment(H0, Hk), m4q.LExperiment(np.eye(9), [np.eye(9)] * 2)):
        with pytest.raises(ValueError):
            exp.feedback_batch(np.zeros((3, 9), complex), ts[:4], _law())        # three intervals, a law of four steps
        with pytest.raises(ValueError):
            exp.feedback_batch(np.zeros((3, 9), complex), ts, _law(), op0=np.zeros((2, 3, 3)))
    with pytest.raises(ValueError):
        m4q.QSynthesis(np.zeros((2, 2)), [np.eye(2)]).feedback_batch(np.zeros((3, 9), complex), ts, _law(m=1))


def test_wrapper_hands_the_kernel_what_it_was_given(monkeypatch):
    """The arguments of the C call: a per-member law with its band and per-member u_prev, a non-uniform grid, per-member sigma and
    a member base, per-member op0 beside shared control operators; then a shared law without band, noise, figure or controls."""
    seen = {}

    class Fake:
        def m4q_plant_feedback_batch(self, *a):
            seen["a"] = a
            return 0

        def m4q_model_feedback_batch(self, *a):
            seen["m"] = a
            return 0

        def m4q_last_error(self):
            return b""
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    B, n, m, N = 3, 9, 2, 4
    rng = np.random.default_rng(9400)
    ts = np.array([0.0, 0.1, 0.35, 0.4, 1.0])
    law = fc.make_law(rng, n, m, N, 0.7, np.zeros(n), members=B)
    assert law.x_ref.shape == (B, N, n)                                                  # (given N + 1 rows: the last is dropped)
    op0 = np.arange(B * 9).reshape(B, 3, 3)
    noise = m4q.MeasurementNoise(np.array([0.1, 0.2, 0.3]), 99, "hermitian", member_base=1000)
    out = m4q.plant_feedback_batch(np.zeros((B, n)), law, op0, np.ones((m, 3, 3)), ts, u_scale=np.ones((B, m)), noise=noise, W=np.eye(n),
                                   target=np.zeros((B, n)), keep="last", figure="all")
    a = seen["a"]
    assert len(a) == 35 and a[:5] == (B, n, m, _lib.PLANT_HAMILTONIAN, N)
    assert np.array_equal(np.ctypeslib.as_array(a[5], (N,)), np.diff(ts))
    assert np.array_equal(np.ctypeslib.as_array(a[7], (B * N * (n + 1) * m * 2,)), law.gains.view(np.float64).reshape(-1))
    assert np.array_equal(np.ctypeslib.as_array(a[8], (B * N * n * 2,)), law.x_ref.view(np.float64).reshape(-1))
    assert np.array_equal(np.ctypeslib.as_array(a[9], (B * N * m,)), law.u_ref.reshape(-1))
    assert a[10] == 1 and a[11] == 0.7 and a[12] == 1 and a[13] == 0.35 and a[15] == 1
    assert np.array_equal(np.ctypeslib.as_array(a[14], (B * m,)), law.u_prev.reshape(-1))
    assert a[16] is not None and a[19] == 1
    assert a[20] == _lib.NOISE_HERMITIAN and a[22] == 1 and a[23] == 99 and a[24] == 1000
    assert np.array_equal(np.ctypeslib.as_array(a[21], (B,)), [0.1, 0.2, 0.3])
    assert a[27] == 1 and a[28] == 1 and a[30] == 2 and a[32] is not None
    assert out["xs"].shape == (B, n) and out["q"].shape == (B, N + 1) and out["us"].shape == (B, N, m)
    assert out["clipped"].shape == (B,) and out["clipped"].dtype == np.int32 and out["status"].dtype == np.int32
    shared = m4q.FeedbackLaw(law.gains[0], law.x_ref[0], law.u_ref[0], np.inf)
    out = m4q.plant_feedback_batch(np.zeros((B, n)), shared, op0[0], np.ones((m, 3, 3)), 0.5, keep="none", controls=False)
    a = seen["a"]
    assert a[10] == 0 and a[11] == np.inf and a[12] == 0 and a[13] == 0.0 and a[14] is None and a[15] == 0 and a[16] is None
    assert a[19] == 0 and a[20] == 0 and a[21] is None and a[25] is None and a[26] is None
    assert a[28] == 0 and a[29] is None and a[30] == 0 and a[31] is None and a[32] is None and a[33] is not None and a[34] is not None
    assert set(out) == {"clipped", "status"}
    one = m4q.MeasurementNoise(0.25, 7)
    out = m4q.model_feedback_batch(np.zeros((B, n)), shared, np.zeros((B, n, 3 * n)), 1, noise=one)
    a = seen["m"]
    assert len(a) == 33 and a[:5] == (B, n, m, 1, N) and a[9] == 0 and a[17] == 1 and a[18] == _lib.NOISE_IID and a[20] == 0
    assert np.ctypeslib.as_array(a[19], (1,))[0] == 0.25 and a[21] == 7 and a[22] == 0
    assert set(out) == {"xs", "us", "clipped", "status"} and out["xs"].shape == (B, N + 1, n)


def test_prototypes_and_exports():
    assert len(_lib.PROTOTYPES["m4q_plant_feedback_batch"][1]) == 35 and len(_lib.PROTOTYPES["m4q_model_feedback_batch"][1]) == 33
    L = _lib.lib()
    assert L.m4q_plant_feedback_batch.argtypes[-1] is IP and L.m4q_model_feedback_batch.argtypes[-2] is IP
    for name in ("FeedbackLaw", "plant_feedback_batch", "model_feedback_batch", "plant_feedback_reference", "model_feedback_reference"):
        assert getattr(m4q, name) is getattr(feedback, name)
    for cls in (m4q.QExperiment, m4q.LExperiment, m4q.QSynthesis):
        assert callable(cls.feedback_batch)
    import sys
    assert "torch" not in sys.modules or "torch" not in feedback.__dict__

"""The robust optimiser (m4q_plant_robust_batch) and its multi rollout (m4q_plant_rollout_multi_batch) without a GPU: the NumPy
definition of mpc4quantum_amd/plant_robust.py - the two-loop recursion against the dense BFGS update, the memoryless loop against a
hand-written projected gradient, convergence on a quadratic, every status, the rejected-with-memory path, descent on the plant
cases - the C++ twin of the direction (csrc/m4q_robust_host.h) bit for bit under the sanitizers, the prototypes, every refusal of
the C ABI before a device is asked for and every ValueError of the wrappers before the library is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from mpc4quantum_amd import plant_robust as pr
from tests import grad_cases as gc
from tests import plant_robust_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
DP, IP = _lib._dp, _lib._ip


# ---------------------------------------------------------------- the direction
def _curved_pairs(rng, shape, count):
    """Pairs (s, y = A s) of one SPD matrix A: every one passes the curvature test."""
    nm = int(np.prod(shape))
    M = rng.standard_normal((nm, nm))
    A = M @ M.T + nm * np.eye(nm)
    out = []
    for _ in range(count):
        s = rng.standard_normal(shape)
        out.append((s, (A @ s.reshape(-1)).reshape(shape)))
    return out


@pytest.mark.parametrize("count", [1, 2, 5, 8])
def test_two_loop_recursion_is_the_dense_bfgs_inverse(count):
    rng = np.random.default_rng(4100 + count)
    shape = (6, 2)
    pairs = _curved_pairs(rng, shape, count)
    pg = rng.standard_normal(shape)
    s, y = pairs[-1]
    H = (np.vdot(s, y) / np.vdot(y, y)) * np.eye(12)
    for s, y in pairs:
        s, y = s.reshape(-1), y.reshape(-1)
        assert s @ y > pr.CURVATURE * np.sqrt((s @ s) * (y @ y))
        rho = 1.0 / (s @ y)
        V = np.eye(12) - rho * np.outer(y, s)
        H = V.T @ H @ V + rho * np.outer(s, s)
    want = (H @ pg.reshape(-1)).reshape(shape)
    got = pr._two_loop(pairs, pg)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ---------------------------------------------------------------- the loop on a quadratic
class Quadratic:
    """F(U) = 1/2 (U - c)^T A (U - c) + f0 on [N, m], A SPD: a pair of callables for evaluate=, with counters."""

    def __init__(self, seed, shape=(5, 2), cond=30.0):
        rng = np.random.default_rng(seed)
        nm = int(np.prod(shape))
        Q, _ = np.linalg.qr(rng.standard_normal((nm, nm)))
        self.A = Q @ np.diag(np.linspace(1.0, cond, nm)) @ Q.T
        self.c = rng.uniform(-1.0, 1.0, shape)
        self.shape, self.grads, self.rolls = shape, 0, 0

    def F(self, U):
        d = (U - self.c).reshape(-1)
        return 0.5 * float(d @ self.A @ d) + 0.25

    def grad(self, U):
        self.grads += 1
        return self.F(U), (self.A @ (U - self.c).reshape(-1)).reshape(self.shape)

    def roll(self, us):
        self.rolls += 1
        return np.array([self.F(u) for u in us])


def _run(q, U0, sat, **kw):
    return m4q.plant_robust_reference(None, U0, None, None, None, None, None, sat, evaluate=(q.grad, q.roll), **kw)


def test_memoryless_loop_is_a_projected_gradient_loop():
    q = Quadratic(4200, cond=4.0)
    sat, step0, steps, iters = 0.6, 0.3, 8, 7
    U0 = np.zeros(q.shape)
    got = _run(q, U0, sat, iters=iters, steps=steps, mem=0, step0=step0, tol=0.0)
    # written out by hand: U <- the best of clip(U - 2^-j (step0 / max|pg|) pg), pg the gradient with the blocked entries zeroed
    U = np.clip(U0, -sat, sat)
    hist, alphas = [q.F(U)], []
    for _ in range(iters):
        F, g = q.F(U), (q.A @ (U - q.c).reshape(-1)).reshape(q.shape)
        pg = np.where(((U == sat) & (g < 0)) | ((U == -sat) & (g > 0)), 0.0, g)
        p = -((step0 / np.abs(pg).max()) * pg)
        trials = [np.clip(U + 2.0 ** -j * p, -sat, sat) for j in range(steps)]
        Fs = [q.F(t) for t in trials]
        j = int(np.argmin(Fs))
        assert Fs[j] < F
        U = trials[j]
        hist.append(Fs[j])
        alphas.append(2.0 ** -j)
    assert np.array_equal(got["U"], U) and np.array_equal(got["cost_hist"], hist) and np.array_equal(got["alpha_hist"], alphas)
    assert got["status"] == pr.STATUS_ITERS and got["n_iter"] == iters and got["cost"] == hist[-1]
    assert np.any(np.abs(U) == sat)                                 # (the box was met)


@pytest.mark.parametrize("mem", [0, 3, 8])
def test_quadratic_converges_and_never_goes_up(mem):
    """(Without memory a trial step's largest entry is step0 2^-j whatever the gradient: close to the minimum none of the 8 lengths
    descends and the run ends with status 2; with memory the steps scale themselves and the run converges.)"""
    q = Quadratic(4300, cond=10.0)
    out = _run(q, np.zeros(q.shape), np.inf, iters=64, steps=8, mem=mem, step0=0.5, tol=1e-13, gtol=1e-9)
    h, a = out["cost_hist"], out["alpha_hist"]
    assert np.all(np.diff(h) <= 0) and h[-1] < h[0]
    assert all(h[i + 1] < h[i] for i in range(out["n_iter"]) if a[i] > 0)
    assert all(h[i + 1] == h[i] for i in range(out["n_iter"]) if a[i] == 0)
    assert out["cost"] == h[-1]
    assert np.all(a[out["n_iter"]:] == 0) and np.all(out["pgrad_hist"][out["n_iter"]:] == 0) and np.all(h[out["n_iter"]:] == h[-1])
    if mem:
        assert out["status"] == pr.STATUS_CONVERGED
        assert np.abs(out["U"] - q.c).max() <= 1e-5 and out["cost"] - 0.25 <= 1e-9
    else:
        # no descent along -g at the shortest length a = 2^-7 step0 / max|g| means a >= 2 |g|^2 / g^T A g >= 2 / cond
        assert out["status"] == pr.STATUS_NO_DESCENT and out["pgrad_hist"][out["n_iter"] - 1] <= 0.5 * 10.0 / 2 ** 8


def test_status_converged_by_gtol_and_by_tol():
    q = Quadratic(4400)
    out = _run(q, np.zeros(q.shape), np.inf, iters=5, steps=4, mem=3, step0=0.1, tol=0.0, gtol=1e6)
    assert (out["status"], out["n_iter"], q.rolls) == (pr.STATUS_CONVERGED, 1, 0) and out["pgrad_hist"][0] > 0
    assert np.all(out["alpha_hist"] == 0) and np.all(out["cost_hist"] == out["cost"])
    q = Quadratic(4400)
    out = _run(q, np.zeros(q.shape), np.inf, iters=5, steps=4, mem=3, step0=0.1, tol=1.0, gtol=0.0)
    assert (out["status"], out["n_iter"]) == (pr.STATUS_CONVERGED, 1) and out["alpha_hist"][0] > 0
    assert out["cost_hist"][1] < out["cost_hist"][0] and np.all(out["cost_hist"][1:] == out["cost"])


def test_status_no_descent_and_not_finite():
    args, kw = rc.own_trajectory_case()
    out = m4q.plant_robust_reference(*args, **kw)
    assert (out["status"], out["n_iter"]) == (pr.STATUS_NO_DESCENT, 1) and 0 < out["cost"] < 1e-15
    assert np.array_equal(out["U"], args[1]) and np.all(out["cost_hist"] == out["cost"]) and np.all(out["alpha_hist"] == 0)
    bad = args[0].copy()
    bad[0, 1] = np.nan
    out = m4q.plant_robust_reference(bad, *args[1:], **kw)
    assert (out["status"], out["n_iter"]) == (pr.STATUS_NOT_FINITE, 0) and np.isnan(out["cost"]) and np.all(np.isnan(out["cost_hist"]))
    assert np.array_equal(out["U"], args[1]) and np.all(out["pgrad_hist"] == 0)


def test_rejected_with_memory_clears_it_and_goes_on_without_a_gradient():
    q = Quadratic(4600)
    calls = []

    def roll(us):
        calls.append(len(us))
        Fs = q.roll(us)
        return Fs + 1e3 if len(calls) == 2 else Fs                  # the second line search finds nothing

    trace = []
    out = m4q.plant_robust_reference(None, np.zeros(q.shape), None, None, None, None, None, np.inf, evaluate=(q.grad, roll), iters=4,
                                     steps=3, mem=4, step0=0.2, tol=0.0, trace=trace)
    assert out["status"] == pr.STATUS_ITERS and out["n_iter"] == 4 and calls == [3, 3, 3, 3]
    assert [t["used"] for t in trace[:3]] == [0, 1, 0] and trace[3]["used"] == 1
    assert out["alpha_hist"][0] > 0 and out["alpha_hist"][1] == 0 and out["alpha_hist"][2] > 0
    assert q.grads == 3                                             # iterations 0, 1 and 3: U did not move in iteration 1
    assert trace[2]["g"] is trace[1]["g"] and out["pgrad_hist"][2] == out["pgrad_hist"][1]
    assert out["cost_hist"][2] == out["cost_hist"][1] and out["cost_hist"][3] < out["cost_hist"][2]


# ---------------------------------------------------------------- the loop on the plants
@pytest.mark.parametrize("mem", [0, 3])
@pytest.mark.parametrize("name", ["4-1", "9-2", "16-1-process"])
def test_accepted_steps_are_descent_directions_of_the_reference_gradient(name, mem):
    k = rc.case(name, 5, 5, 4700 + rc.NAMES.index(name))
    trace = []
    out = m4q.plant_robust_reference(*k["args"], figure="sum", iters=4, steps=4, mem=mem, step0=rc.STEP0, tol=0.0, trace=trace,
                                     members=True, **k["kw"])
    x0, _, op0, ops, ts, W, f, _ = k["args"]
    accepted = [t for t in trace if t["j"] is not None]
    assert accepted and len(trace) <= out["n_iter"]          # (an iteration that stops on gtol rolls nothing)
    for t in accepted:
        ref = m4q.plant_rollout_grad_reference(x0, t["U"], op0, ops, ts, W, f, figure="sum", reduce=True, **k["kw"])
        assert np.array_equal(ref["grad"], t["g"]) and ref["q_mean"] == t["F"]
        assert float(np.vdot(t["p"], ref["grad"])) < 0 and t["Fs"][t["j"]] < t["F"]
    assert out["cost"] < out["cost_hist"][0] and np.all(np.abs(out["U"]) <= k["args"][7])
    if mem:
        assert max(t["used"] for t in trace) >= 1                   # (the memory was in use)
    # the members' objectives at U: their ordered mean is the cost, bit for bit
    assert out["J"].shape == (5,) and float(m4q.ordered_weighted_sum(out["J"], k["kw"]["weights"])) == out["cost"]
    again = m4q.plant_rollout_grad_reference(x0, out["U"], op0, ops, ts, W, f, figure="sum", reduce=True, **k["kw"])
    assert again["q_mean"] == out["cost"]


@pytest.mark.parametrize("mem", [0, 3])
@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("name", rc.NAMES)
def test_a_gradient_pushed_by_its_bound_changes_no_decision(name, figure, mem):
    """The seeds of the device's comparison with the NumPy definition (tests/test_gpu_plant_robust.py): on them the definition takes
    the same decisions when every gradient is pushed by the project's gradient bound."""
    plain, pushed = rc.definition_runs(name, figure, mem)
    assert np.array_equal(plain["alpha_hist"], pushed["alpha_hist"])
    assert (plain["status"], plain["n_iter"]) == (pushed["status"], pushed["n_iter"]) and np.count_nonzero(plain["alpha_hist"]) >= 2
    dU, dF = rc.movement(plain, pushed)
    print("%s %s mem %d: the pushed run moved U by %.2e and cost_hist by %.2e" % (name, figure, mem, dU, dF))
    assert dU <= 1e-6 and dF <= 1e-6                                # (what moves is of the order of the push, 1e-10)


def test_multi_reference_is_the_gradient_reference_forward():
    k = rc.case("9-2", 3, 4, 4800)
    x0, U0, op0, ops, ts, W, f, sat = k["args"]
    us = np.stack([U0, 0.5 * U0, -U0])
    for figure in ("last", "sum"):
        out = m4q.plant_rollout_multi_reference(x0, us, op0, ops, ts, W, f, figure=figure, **k["kw"])
        assert out["J"].shape == (3, 3) and out["F"].shape == (3,)
        for s in range(3):
            ref = m4q.plant_rollout_grad_reference(x0, us[s], op0, ops, ts, W, f, figure=figure, reduce=True, **k["kw"])
            assert ref["q_mean"] == out["F"][s]


# ---------------------------------------------------------------- the C++ twin of the direction
def _hex(v):
    return " ".join(float(x).hex() for x in np.ravel(v))


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def _direction_cases():
    """(nm-shaped U, g, pairs, pending, sat, step0, mem, steps) - and what each is there for."""
    rng = np.random.default_rng(4900)
    shape = (7, 2)
    cases = []

    def add(why, U, g, pairs, pending, sat, step0, mem, steps=4):
        cases.append(dict(why=why, U=U, g=g, pairs=pairs, pending=pending, sat=sat, step0=step0, mem=mem, steps=steps))
    U = rng.uniform(-0.4, 0.4, shape)
    g = rng.standard_normal(shape)
    add("empty memory", U, g, [], None, 0.5, 0.1, 3)
    add("three pairs, free box", U, g, _curved_pairs(rng, shape, 3), None, np.inf, 0.1, 3, steps=8)
    Ub = U.copy()
    Ub[0, 0], Ub[2, 1], Ub[3, 0], Ub[5, 1] = 0.5, -0.5, 0.5, -0.5
    gb = g.copy()
    gb[0, 0], gb[2, 1], gb[3, 0], gb[5, 1] = -1.0, 2.0, 1.5, -0.5      # two blocked, two at a bound and free to leave it
    add("active bounds, memory", Ub, gb, _curved_pairs(rng, shape, 2), None, 0.5, 0.3, 4)
    add("active bounds, no memory", Ub, gb, [], None, 0.5, 2.0, 0, steps=3)
    s = rng.standard_normal(shape)
    add("a pending pair that fails the curvature test", U, g, _curved_pairs(rng, shape, 2), (s, g + 0.3 * s), 0.5, 0.1, 3)
    add("a pending pair that passes and pushes the oldest out", U, g, _curved_pairs(rng, shape, 2), (s, g - 0.7 * s), 0.5, 0.1, 2)
    add("a pending pair into an empty memory of size 0", U, g, [], (s, g - 0.7 * s), 0.5, 0.1, 0)
    sb, yb = rng.standard_normal(shape), rng.standard_normal(shape)
    if pr._dot(sb, yb) > 0:
        yb = -yb
    add("no descent direction: the memory is cleared", U, g, [(sb, yb)], None, 0.5, 0.1, 3)
    return cases


def _definition(c):
    pairs = list(c["pairs"])
    active, pg, gmax = pr._project(c["U"], c["g"], c["sat"])
    if c["pending"] is not None:
        pr._absorb(pairs, c["pending"][0], c["g"], c["pending"][1], c["mem"])
    p = pr._direction(pairs, c["g"], active, pg, gmax, c["step0"])
    return len(pairs), gmax, p, pr._candidates(c["U"], p, c["sat"], c["steps"])


def test_cpp_direction_equals_the_definition_bit_for_bit_under_sanitizers(tmp_path):
    cases = _direction_cases()
    want = [_definition(c) for c in cases]
    by = {c["why"]: w for c, w in zip(cases, want)}
    # the cases are what they claim to be
    assert by["a pending pair that fails the curvature test"][0] == 2 and by["a pending pair that passes and pushes the oldest out"][0] == 2
    assert by["a pending pair into an empty memory of size 0"][0] == 0 and by["no descent direction: the memory is cleared"][0] == 0
    assert by["three pairs, free box"][0] == 3 and by["active bounds, memory"][0] == 2
    for why in ("active bounds, memory", "active bounds, no memory"):
        p = by[why][2]
        assert p[0, 0] == 0 and p[2, 1] == 0 and p[3, 0] < 0 and p[5, 1] > 0
    lines = [str(len(cases))]
    for c in cases:
        lines.append("%d %d %d %s %s" % (c["U"].size, c["mem"], c["steps"], float(c["sat"]).hex(), float(c["step0"]).hex()))
        lines += [_hex(c["U"]), _hex(c["g"]), str(len(c["pairs"]))]
        for s, y in c["pairs"]:
            lines += [_hex(s), _hex(y)]
        lines.append("0" if c["pending"] is None else "1")
        if c["pending"] is not None:
            lines += [_hex(c["pending"][0]), _hex(c["pending"][1])]
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "direction_driver")
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "mpc4quantum_amd", "csrc"), os.path.join(ROOT, "tests", "robust_host", "direction_driver.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0 and not run.stderr, run.stderr[-4000:]
    out = iter(run.stdout.splitlines())
    for c, (left, gmax, p, cands) in zip(cases, want):
        assert next(out).split() == ["K", str(left)], c["why"]
        assert float.fromhex(next(out).split()[1]) == gmax, c["why"]
        got = np.array([float.fromhex(t) for t in next(out).split()[1:]])
        assert np.array_equal(_bits(got), _bits(p).reshape(-1)), c["why"]
        for j in range(c["steps"]):
            f = next(out).split()
            assert f[:2] == ["C", str(j)]
            got = np.array([float.fromhex(t) for t in f[2:]])
            assert np.array_equal(_bits(got), _bits(cands[j]).reshape(-1)), (c["why"], j)
    assert next(out, None) is None


# ---------------------------------------------------------------- prototypes and exports
@pytest.mark.parametrize("symbol,count", [("m4q_plant_rollout_multi_batch", 20), ("m4q_plant_robust_batch", 32)])
def test_header_and_prototype_table_agree(symbol, count):
    header = open(os.path.join(ROOT, "include", "m4q.h")).read()
    decl = re.search(r"M4Q_API int %s\((.*?)\);" % symbol, header, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double, "const double*": DP, "double*": DP, "int32_t*": IP}
    mine = [ctype[p.rsplit(" ", 1)[0]] for p in params]
    restype, argtypes = _lib.PROTOTYPES[symbol]
    assert restype is ctypes.c_int and argtypes == mine and len(mine) == count
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), symbol)


def test_exports():
    for name in ("plant_rollout_multi_batch", "plant_rollout_multi_reference", "plant_robust_batch", "plant_robust_reference"):
        assert getattr(m4q, name) is getattr(pr, name)
    for cls in (m4q.QExperiment, m4q.LExperiment, m4q.QSynthesis):
        assert callable(cls.robust_batch)


# ---------------------------------------------------------------- the C entry points
def _buf(n, dtype=np.float64):
    a = np.zeros(max(int(n), 1), dtype=dtype)
    return a, a.ctypes.data_as(IP if dtype == np.int32 else DP)


class _Call:
    def _b(self, name, count, dtype=np.float64):
        self.keep[name], p = _buf(count, dtype)
        return p

    def weights(self, values):
        self.keep["w"] = np.array(values, dtype=np.float64)
        return self.keep["w"].ctypes.data_as(DP)

    def __call__(self, **change):
        v = dict(self.v, **change)
        return getattr(_lib.lib(), self.SYMBOL)(*[v[k] for k in self.ORDER])


class _MultiCall(_Call):
    """One valid m4q_plant_rollout_multi_batch call on host buffers of the right sizes; fields are replaced one at a time."""
    SYMBOL = "m4q_plant_rollout_multi_batch"
    ORDER = ("B", "n", "m", "kind", "N", "dts", "x0", "S", "us", "u_scale", "op0", "ops", "per", "W", "target", "t_per", "q_mode",
             "weights", "J", "F")

    def __init__(self, B=3, n=9, m=2, kind=_lib.PLANT_HAMILTONIAN, N=4, k=3, S=3):
        self.keep = {}
        self.v = dict(B=B, n=n, m=m, kind=kind, N=N, dts=self._b("dts", N), x0=self._b("x0", 2 * B * n), S=S, us=self._b("us", 8 * N * m),
                      u_scale=None, op0=self._b("op0", 2 * k * k), ops=self._b("ops", 2 * m * k * k), per=0, W=self._b("W", 2 * n * n),
                      target=self._b("f", 2 * n), t_per=0, q_mode=2, weights=None, J=self._b("J", 8 * B), F=self._b("F", 8))


class _RobustCall(_Call):
    """... and one valid m4q_plant_robust_batch call."""
    SYMBOL = "m4q_plant_robust_batch"
    ORDER = ("B", "n", "m", "kind", "N", "dts", "x0", "U0", "u_scale", "op0", "ops", "per", "W", "target", "t_per", "q_mode", "weights",
             "sat", "iters", "steps", "mem", "step0", "tol", "gtol", "U", "cost", "cost_hist", "alpha_hist", "pgrad_hist", "n_iter",
             "status", "J")

    def __init__(self, B=3, n=9, m=2, kind=_lib.PLANT_HAMILTONIAN, N=4, k=3):
        self.keep = {}
        self.v = dict(B=B, n=n, m=m, kind=kind, N=N, dts=self._b("dts", N), x0=self._b("x0", 2 * B * n), U0=self._b("U0", N * m),
                      u_scale=None, op0=self._b("op0", 2 * k * k), ops=self._b("ops", 2 * m * k * k), per=0, W=self._b("W", 2 * n * n),
                      target=self._b("f", 2 * n), t_per=0, q_mode=1, weights=None, sat=1.0, iters=2, steps=3, mem=2, step0=0.1, tol=1e-9,
                      gtol=0.0, U=self._b("U", N * m), cost=self._b("cost", 1), cost_hist=self._b("ch", 65), alpha_hist=self._b("ah", 64),
                      pgrad_hist=self._b("ph", 64), n_iter=self._b("ni", 1, np.int32), status=self._b("st", 1, np.int32),
                      J=self._b("J", B))


SHARED_BAD = [dict(B=0), dict(B=-2), dict(N=0), dict(N=-1), dict(x0=None), dict(W=None), dict(target=None), dict(q_mode=0),
              dict(q_mode=3), dict(q_mode=-1), dict(dts=None), dict(op0=None), dict(ops=None), dict(kind=0), dict(kind=4), dict(kind=-1),
              dict(kind=_lib.PLANT_PROCESS)]
MULTI_BAD = SHARED_BAD + [dict(us=None), dict(S=0), dict(S=9), dict(S=-1), dict(J=None, F=None)]
ROBUST_BAD = SHARED_BAD + [dict(U0=None), dict(U=None), dict(cost=None), dict(cost_hist=None), dict(alpha_hist=None), dict(pgrad_hist=None),
                           dict(n_iter=None), dict(status=None), dict(sat=0.0), dict(sat=-1.0), dict(sat=np.nan), dict(iters=0),
                           dict(iters=65), dict(steps=0), dict(steps=9), dict(mem=-1), dict(mem=9), dict(step0=0.0), dict(step0=-0.1),
                           dict(step0=np.inf), dict(step0=np.nan), dict(tol=-1e-9), dict(tol=np.inf), dict(tol=np.nan),
                           dict(gtol=-1e-9), dict(gtol=np.inf), dict(gtol=np.nan)]
BAD_WEIGHTS = [[1.0, np.nan, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -1e-300], [-1.0, 1.0, 1.0]]


@pytest.mark.parametrize("change", MULTI_BAD, ids=str)
def test_multi_rollout_refuses_bad_arguments(change):
    """(kind = PROCESS on n = 9: not a fourth power.)"""
    assert _MultiCall()(**change) == _lib.E_BADARG
    assert b"m4q_plant_rollout_multi_batch" in _lib.lib().m4q_last_error()


@pytest.mark.parametrize("change", ROBUST_BAD, ids=str)
def test_robust_refuses_bad_arguments(change):
    assert _RobustCall()(**change) == _lib.E_BADARG
    assert b"m4q_plant_robust_batch" in _lib.lib().m4q_last_error()


@pytest.mark.parametrize("values", BAD_WEIGHTS, ids=str)
def test_both_refuse_bad_weights(values):
    for call in (_MultiCall(), _RobustCall()):
        assert call(weights=call.weights(values)) == _lib.E_BADARG
    m = _MultiCall()
    assert m(weights=m.weights(values), F=None) == _lib.E_BADARG     # (checked even where no mean is asked for)


@pytest.mark.parametrize("Call", [_MultiCall, _RobustCall])
def test_both_refuse_what_has_no_kernel(Call):
    assert Call(n=25, k=5)() == _lib.E_UNSUPPORTED                             # no compiled shape
    assert Call(n=9, m=3)() == _lib.E_UNSUPPORTED
    assert Call(n=8, m=2, k=2)() == _lib.E_UNSUPPORTED                         # a shape with a model and no device plant
    assert Call(n=9, kind=_lib.PLANT_GENERATOR, k=9)() == _lib.E_UNSUPPORTED   # the generator plant, with the gradient's advice
    err = _lib.lib().m4q_last_error()
    assert b"generator" in err and b"m4q_model_rollout_grad_batch" in err and Call.SYMBOL.encode() in err
    assert Call(n=4, m=1, kind=_lib.PLANT_GENERATOR, k=4)() == _lib.E_UNSUPPORTED


def test_well_formed_calls_reach_the_device():
    """Every check passed: the call asks for a device (and, where there is one, runs on the all-zero data)."""
    want = 0 if _lib.device_count() > 0 else _lib.E_NODEVICE
    assert _MultiCall()() == want
    assert _MultiCall()(S=1, q_mode=1, F=None) == want and _MultiCall()(S=8, J=None) == want
    m = _MultiCall()
    assert m(weights=m.weights([0.0, 1.0, 2.5])) == want
    assert _MultiCall(n=16, m=2, k=4)() == want                               # the plant-only shape serves both
    assert _MultiCall(n=16, m=1, kind=_lib.PLANT_PROCESS, k=2)() == want
    assert _RobustCall()() == want
    assert _RobustCall()(J=None, q_mode=2, mem=0, iters=64, steps=8, sat=np.inf) == want
    assert _RobustCall(n=16, m=2, k=4)() == want
    assert _RobustCall(n=16, m=3, kind=_lib.PLANT_PROCESS, k=2)() == want


# ---------------------------------------------------------------- the Python wrappers
@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library is a failure: shapes are refused before it is loaded."""
    def boom():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _args(B=3, n=9, m=2, N=4, k=3, **more):
    return dict(more, x0=np.zeros((B, n), complex), op0=np.zeros((k, k), complex), ops=np.zeros((m, k, k), complex), dt_or_ts=0.25, W=np.eye(n),
                target=np.zeros(n))


SHAPES_BAD = [dict(x0=np.zeros(9)), dict(x0=np.zeros((0, 9))), dict(u_scale=np.ones((3, 1))), dict(u_scale=np.ones(2)), dict(W=None),
              dict(target=None), dict(W=np.eye(4)), dict(target=np.zeros(4)), dict(target=np.zeros((2, 9))), dict(figure="all"),
              dict(figure="none"), dict(weights=np.ones(2)), dict(weights=[1.0, np.nan, 1.0]), dict(weights=[1.0, -1.0, 1.0]),
              dict(op0=np.zeros((2, 2))), dict(ops=np.zeros((1, 3, 3))), dict(dt_or_ts=np.zeros(4)), dict(dt_or_ts=np.inf), dict(kind=0),
              dict(kind=_lib.PLANT_PROCESS), dict(kind=_lib.PLANT_GENERATOR)]


def _ident(c):
    return ",".join("%s%s" % (k, getattr(v, "shape", v)) for k, v in c.items())


@pytest.mark.parametrize("change", SHAPES_BAD + [dict(us=np.zeros(4)), dict(us=np.zeros((9, 4, 2))), dict(us=np.zeros((2, 3, 4, 2))),
                                                 dict(us=np.zeros((0, 4, 2))), dict(members=False, mean=False)], ids=_ident)
def test_multi_wrapper_refuses_bad_arguments(no_library, change):
    with pytest.raises(ValueError):
        m4q.plant_rollout_multi_batch(**dict(_args(us=np.zeros((3, 4, 2))), **change))


@pytest.mark.parametrize("change", SHAPES_BAD + [dict(U0=np.zeros(4)), dict(U0=np.zeros((3, 4, 2))), dict(sat=0.0), dict(sat=np.nan),
                                                 dict(iters=0), dict(iters=65), dict(steps=0), dict(steps=9), dict(mem=-1), dict(mem=9),
                                                 dict(step0=0.0), dict(step0=np.inf), dict(tol=-1.0), dict(tol=np.nan), dict(gtol=-1.0),
                                                 dict(gtol=np.inf)], ids=_ident)
def test_robust_wrapper_refuses_bad_arguments(no_library, change):
    with pytest.raises(ValueError):
        m4q.plant_robust_batch(**dict(_args(U0=np.zeros((4, 2)), sat=1.0), **change))
    if "kind" not in change or change["kind"] == _lib.PLANT_GENERATOR:
        with pytest.raises(ValueError):
            m4q.plant_robust_reference(**dict(_args(U0=np.zeros((4, 2)), sat=1.0), **change))


def test_integer_parameters_must_be_integers(no_library):
    for change in (dict(iters=2.5), dict(steps=True), dict(mem=1.5)):
        with pytest.raises(TypeError):
            m4q.plant_robust_batch(**dict(_args(U0=np.zeros((4, 2)), sat=1.0), **change))


def test_experiment_wrappers_refuse_before_the_library(no_library):
    x0 = np.zeros((3, 9), complex)
    exp = m4q.QExperiment(np.diag([0.0, 1.0, 2.0]), [np.eye(3), np.eye(3)])
    with pytest.raises(ValueError):
        exp.robust_batch(x0, np.zeros((4, 3)), 0.25, np.eye(9), np.zeros(9), 1.0)          # three controls for two operators
    with pytest.raises(ValueError):
        exp.robust_batch(x0, np.zeros((4, 2)), 0.25, np.eye(9), np.zeros(9), 1.0, mem=9)
    with pytest.raises(ValueError, match="model_rollout_grad_batch"):
        m4q.LExperiment(np.eye(9), [np.eye(9)] * 2).robust_batch(x0, np.zeros((4, 2)), 0.25, np.eye(9), np.zeros(9), 1.0)
    with pytest.raises(ValueError):
        m4q.QSynthesis(np.zeros((2, 2)), [np.eye(2)]).robust_batch(x0, np.zeros((4, 1)), 0.25, np.eye(9), np.zeros(9), 1.0)


def test_wrappers_hand_the_library_what_they_were_given(monkeypatch):
    seen = {}

    class Fake:
        def m4q_plant_rollout_multi_batch(self, *a):
            seen["multi"] = a
            return 0

        def m4q_plant_robust_batch(self, *a):
            seen["robust"] = a
            return 0

        def m4q_last_error(self):
            return b""
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    B, n, m, N = 3, 9, 2, 4
    ts = np.array([0.0, 0.1, 0.35, 0.4, 1.0])
    us = np.arange(2 * N * m, dtype=float).reshape(2, N, m)
    op0 = np.arange(B * 9).reshape(B, 3, 3)
    out = m4q.plant_rollout_multi_batch(np.zeros((B, n)), us, op0, np.ones((m, 3, 3)), ts, np.eye(n), np.zeros((B, n)),
                                        u_scale=np.ones((B, m)), figure="sum", weights=[1.0, 2.0, 3.0])
    a = seen["multi"]
    assert len(a) == 20 and a[:5] == (B, n, m, _lib.PLANT_HAMILTONIAN, N) and a[7] == 2
    assert np.array_equal(np.ctypeslib.as_array(a[5], (N,)), np.diff(ts)) and np.array_equal(np.ctypeslib.as_array(a[8], (2, N, m)), us)
    assert a[9] is not None and a[12] == 1 and a[15] == 1 and a[16] == 2
    assert np.array_equal(np.ctypeslib.as_array(a[17], (B,)), [1.0, 2.0, 3.0])
    assert out["J"].shape == (B, 2) and out["F"].shape == (2,)
    out = m4q.plant_rollout_multi_batch(np.zeros((B, n)), us[0], op0[0], np.ones((m, 3, 3)), 0.5, np.eye(n), np.zeros(n), members=False)
    a = seen["multi"]
    assert a[7] == 1 and a[9] is None and a[12] == 0 and a[15] == 0 and a[16] == 1 and a[17] is None and a[18] is None
    assert set(out) == {"F"} and out["F"].shape == (1,)
    out = m4q.plant_robust_batch(np.zeros((B, n)), us[1], op0, np.ones((m, 3, 3)), ts, np.eye(n), np.zeros(n), np.inf, figure="sum",
                                 iters=7, steps=5, mem=0, step0=0.25, tol=1e-7, gtol=1e-3, members=True)
    a = seen["robust"]
    assert len(a) == 32 and a[:5] == (B, n, m, _lib.PLANT_HAMILTONIAN, N)
    assert np.array_equal(np.ctypeslib.as_array(a[7], (N, m)), us[1]) and a[8] is None and a[11] == 1 and a[14] == 0 and a[15] == 2
    assert a[16] is None and a[17:24] == (np.inf, 7, 5, 0, 0.25, 1e-7, 1e-3) and a[31] is not None
    assert out["U"].shape == (N, m) and out["cost_hist"].shape == (8,) and out["alpha_hist"].shape == (7,)
    assert out["pgrad_hist"].shape == (7,) and out["J"].shape == (B,) and isinstance(out["cost"], float)
    assert isinstance(out["n_iter"], int) and isinstance(out["status"], int)
    out = m4q.plant_robust_batch(np.zeros((B, n)), us[1], op0, np.ones((m, 3, 3)), ts, np.eye(n), np.zeros(n), 1.0)
    assert seen["robust"][31] is None and "J" not in out

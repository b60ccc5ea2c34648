"""What the tests of the feedback runs share (tests/test_feedback_host.py, tests/test_gpu_feedback.py): the plant cases of the
rollout tests, seeded laws whose bounds are active, an independent closed loop of a few lines (the oracle's plant steps, np.clip),
and the per-step residuals of a stored run."""
import numpy as np

from mpc4quantum_amd import FeedbackLaw, _lib
from tests import grad_cases as gc
from tests.test_gpu_rollout import CASES, _grid, case  # noqa: F401  (the six plant cases, their operators and reference steps)

PLANTS = list(CASES)


def make_law(rng, n, m, N, sat, x_near, members=None, band=True):
    """A law with bounds that bite: gains of the order of sat per unit of state error, references within 1.3 sat, a band of half
    the box around a u_prev inside it.  x_near [n]: a state of the ensemble, the reference trajectory stays near it."""
    lead = () if members is None else (members,)
    gains = 0.6 * sat * (rng.standard_normal(lead + (N, n + 1, m)) + 1j * rng.standard_normal(lead + (N, n + 1, m)))
    x_ref = x_near + 0.1 * (rng.standard_normal(lead + (N + 1, n)) + 1j * rng.standard_normal(lead + (N + 1, n)))
    u_ref = rng.uniform(-1.3 * sat, 1.3 * sat, lead + (N, m))
    if not band:
        return FeedbackLaw(gains, x_ref, u_ref, sat)
    return FeedbackLaw(gains, x_ref, u_ref, sat, du=0.5 * sat, u_prev=rng.uniform(-0.5 * sat, 0.5 * sat, lead + (m,)))


def law_terms(law, xs, us):
    """Per (b, t): the law evaluated in NumPy on stored states xs [B, N + 1, n], with p the stored control before (us [B, N, m]).
    Returns u, s, lo, hi [B, N, m] and the magnitude the dot product's rounding scales with, sum_j |K||d| + |k0| + |ubar|."""
    B, N = us.shape[:2]
    out = [np.empty(us.shape) for _ in range(5)]
    for b in range(B):
        for t in range(N):
            p = law.prev(b) if t == 0 else us[b, t - 1]
            vals = law.terms(t, xs[b, t], p, b)
            i = b if law.members is not None else ()
            K = law.gains[i][t]
            mag = np.abs(K[:law.n]).T @ np.abs(xs[b, t] - law.x_ref[i][t]) + np.abs(K[law.n]) + np.abs(law.u_ref[i][t])
            for o, v in zip(out, vals + (mag,)):
                o[b, t] = v
    return out


def activity(law, u, s, lo, hi):
    """How many (b, t, k) of a run sit at the lower bound, at the upper bound, inside, and at a bound the band set."""
    low, up = s <= lo, s >= hi
    banded = (low & (lo > -law.sat)) | (up & (hi < law.sat))
    return dict(lower=int(low.sum()), upper=int(up.sum()), interior=int((~low & ~up).sum()), band=int(banded.sum()))


def independent_plant_run(c, x0, law, op0, ops, dts, sc, noise=None):
    """The closed loop written out: c.step (the oracle's plant steps, a few lines of expm for the process plant) and the law with
    np.clip.  op0 / ops [B, ...], sc [B, m].  Returns xs [B, N + 1, n], us [B, N, m], clipped [B]."""
    B, n, N, m = x0.shape[0], law.n, law.N, law.m
    xs, us, clipped = np.empty((B, N + 1, n), complex), np.empty((B, N, m)), np.zeros(B, int)
    for b in range(B):
        i = b if law.members is not None else ()
        x = xs[b, 0] = x0[b]
        p = law.prev(b)
        for t in range(N):
            K = law.gains[i][t]
            s = np.array([sum((K[j, k] * (x[j] - law.x_ref[i][t, j])).real for j in range(n)) + K[n, k].real + law.u_ref[i][t, k]
                          for k in range(m)])
            lo, hi = -law.sat * np.ones(m), law.sat * np.ones(m)
            if law.du is not None:
                lo, hi = np.maximum(lo, p - law.du), np.minimum(hi, p + law.du)
            u = np.clip(s, lo, hi)
            clipped[b] += int(((s <= lo) | (s >= hi)).sum())
            x = c.step(x, sc[b] * u, op0[b], list(ops[b]), dts[t])
            if noise is not None:
                x = x + noise.sample([b], t + 1, n)[0]
            xs[b, t + 1], us[b, t], p = x, u, u
    return xs, us, clipped


def step_residuals(step, xs, us, sc, noise=None):
    """xs[b][t + 1] - step(b, t, xs[b][t], sc[b] us[b][t]) (minus the noise of (b, t + 1)) for a stored run, [B, N, n]."""
    B, N = us.shape[:2]
    res = np.empty((B, N, xs.shape[2]), complex)
    for b in range(B):
        for t in range(N):
            res[b, t] = xs[b, t + 1] - step(b, t, xs[b, t], sc[b] * us[b, t])
            if noise is not None:
                res[b, t] -= noise.sample([b], t + 1, xs.shape[2])[0]
    return res


def figures(xs, W, f):
    return gc.figures(xs, W, f)


def kind_name(kind):
    return {_lib.PLANT_HAMILTONIAN: "hamiltonian", _lib.PLANT_GENERATOR: "generator", _lib.PLANT_PROCESS: "process"}[int(kind)]

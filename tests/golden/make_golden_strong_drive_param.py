"""Generate tests/golden/strong_drive_param_truth.npz: the truth of the plant-parameter gradient on every (case, direction set) of
tests/strong_drive_cases.py (all_param_pairs), computed with mpmath at 40 digits and rounded to fp64.

    python tests/golden/make_golden_strong_drive_param.py

As make_golden_strong_drive.py (whose helpers this imports, and whose file it does not touch): nothing goes through SciPy's expm or
the package's kernels or definitions.  The exponent of every (member, step) is formed in 40-digit arithmetic from the case's fp64
inputs, and the derivative of a step comes ONE DIRECTION AT A TIME from the upper right block of expm([[X, E], [0, X]]), 2d x 2d -
not from the (1 + p_tot) d block matrix of the kernels and of the definition.  E_j = -i dts[t] D_j for the p directions, and
E = -i dts[t] u[t][k] H_k (the unscaled control) for the drive gains.

The adjoint pass is the one of mpc4quantum_amd/plant_param.py's docstring: J = sum_t col_w[t] q_t against the data, a column of
weight 0 skipped (its data never read); lam_N = col_w[N] g_N, and for t = N - 1 .. 0
    grad[e] += Re(lam_{t+1}^H dx_{t+1}/dz_e),    lam_t = U^H Lam_{t+1} U + col_w[t] g_t
(columns of weight 0 still propagate the costate).

Per pair "<cell>-<variant>-B<B>-N<N>/p<p>[+gains]/<field>":
    J           [B]
    grad_theta  [B, p]
    grad_scale  [B, m]      (sets with the gains)
tests/test_strong_drive_host.py recomputes two cells with compute() and requires the stored bits."""
import importlib.util
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from mpc4quantum_amd import _lib  # noqa: E402
from tests import strong_drive_cases as sd  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_strong_drive", os.path.join(HERE, "make_golden_strong_drive.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

DIGITS = mg.DIGITS


def compute(pr):
    """The truth of one (case, set): {field: fp64 array}."""
    with mp.workdps(DIGITS):
        return _compute(pr)


def _compute(pr):
    cs = pr.cs
    B, N, m, d, p = cs.B, cs.N, cs.m, cs.d, pr.p
    cols = 1 if cs.kind == _lib.PLANT_HAMILTONIAN else d * d
    W = mg._lift(cs.W)
    S = W + mg._conj(W).T
    cw = [mp.mpf(float(w)) for w in pr.weights()]
    zero = np.zeros((d, d), dtype=object) + mp.mpc(0)
    out = {"J": np.empty(B), "grad_theta": np.empty((B, p))}
    if pr.sg:
        out["grad_scale"] = np.empty((B, m))
    for b in range(B):
        op0, ops = cs.member_ops(b)
        op0, ops = mg._lift(op0), [mg._lift(h) for h in ops]
        Ds = [mg._lift(D) for D in pr.member_dirs(b)]
        sc = [mp.mpf(float(s)) for s in cs.scale(b)]
        u = [[mp.mpf(float(x)) for x in row] for row in cs.useq(b)]
        y = pr.member_data(b)
        xs = [mg._lift(cs.x0[b])]
        Us, dUs = [], []
        for t in range(N):
            G = op0
            for k in range(m):
                G = G + ops[k] * (sc[k] * u[t][k])
            fac = mp.mpc(0, -1) * mp.mpf(float(cs.dts[t]))
            X = G * fac
            Es = [D * fac for D in Ds] + ([ops[k] * (fac * u[t][k]) for k in range(m)] if pr.sg else [])
            U = mg._expm(X)
            Us.append(U)
            dUs.append([mg._expm(np.block([[X, E], [zero, X]]))[:d, d:] for E in Es])
            xs.append(mg._sandwich(U, xs[-1].reshape(d, d, cols), U).reshape(-1))
        J = mp.mpf(0)
        gts = [None] * (N + 1)
        for t in range(N + 1):
            if cw[t] != 0:
                q, gts[t] = mg._figure(xs[t], W, S, mg._lift(y[t]))
                J = J + cw[t] * q
        out["J"][b] = float(J)
        g = [mp.mpf(0)] * pr.p_tot
        lam = gts[N] * cw[N] if cw[N] != 0 else np.zeros(cs.n, dtype=object) + mp.mpc(0)
        for t in range(N - 1, -1, -1):
            R = xs[t].reshape(d, d, cols)
            for e in range(pr.p_tot):
                dx = (mg._sandwich(dUs[t][e], R, Us[t]) + mg._sandwich(Us[t], R, dUs[t][e])).reshape(-1)
                g[e] = g[e] + mp.re(np.dot(mg._conj(lam), dx))
            Ut = mg._conj(Us[t]).T
            lam = mg._sandwich(Ut, lam.reshape(d, d, cols), Ut).reshape(-1)
            if cw[t] != 0:
                lam = lam + gts[t] * cw[t]
        out["grad_theta"][b] = [float(x) for x in g[:p]]
        if pr.sg:
            out["grad_scale"][b] = [float(x) for x in g[p:]]
    return out


def main():
    data = {}
    for key in sd.all_param_pairs():
        pr = sd.param_case(*key)
        for field, a in compute(pr).items():
            data[pr.id + "/" + field] = a
        print(pr.id, flush=True)
    np.savez_compressed(sd.PARAM_TRUTH_FILE, **data)
    print("wrote %s: %d arrays, %d bytes" % (sd.PARAM_TRUTH_FILE, len(data), os.path.getsize(sd.PARAM_TRUTH_FILE)))


if __name__ == "__main__":
    main()

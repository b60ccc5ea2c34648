"""Generate tests/golden/strong_drive_truth.npz: the truth of every case of tests/strong_drive_cases.py, computed with mpmath at
40 digits and rounded to fp64.

    python tests/golden/make_golden_strong_drive.py

Nothing here goes through SciPy's expm or any code of the package's kernels or definitions: the exponent of every (member, step) is
formed in 40-digit arithmetic from the case's fp64 inputs (the controls a member sees are u_scale * u, exactly), exponentiated by
mpmath, and everything after it - the state chain, the figures, the adjoint pass - is 40-digit arithmetic on NumPy object arrays.

Per case "<cell>-<variant>-B<B>-N<N>/<field>":
  Hamiltonian and process plants
    U         [B, N, d, d]     expm(X), X = -i dts[t] (H0 + sum_k v_k H_k)
    dU        [B, N, m, d, d]  the Frechet derivative L(X, -i dts[t] H_k): the upper right block of expm([[X, E_k], [0, X]]), one
                               control at a time (not the (1 + m) d block matrix of the kernels)
    xs        [B, N + 1, n]    the state chain from x0
    q         [B, N + 1]       Re((x_t - f)^H W (x_t - f))
    J_sum     [B]              sum_t q_t
    grad_last, grad_sum [B, N, m]   dJ/du[t][k] for J = q_N and J = sum_t q_t (with respect to the unscaled controls)
    gs_last, gs_sum     [B, m]      dJ/du_scale[b][k]
  generator plant
    xs, q, J_sum              the propagated states expm(dts[t] L(v_t)) x_t and their figures
tests/test_strong_drive_host.py recomputes two cells with compute() and requires the stored bits."""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from mpc4quantum_amd import _lib  # noqa: E402
from tests import strong_drive_cases as sd  # noqa: E402

DIGITS = 40

_lift = np.vectorize(lambda z: mp.mpc(complex(z).real, complex(z).imag), otypes=[object])
_conj = np.vectorize(lambda z: mp.conj(z), otypes=[object])
_cplx = np.vectorize(lambda z: complex(z), otypes=[np.complex128])


def _expm(A):
    r, c = A.shape
    return np.array(mp.expm(mp.matrix(A.tolist())).tolist(), dtype=object).reshape(r, c)


def _sandwich(P, R, Q):
    """einsum('ac,cgx,eg->aex', P, R, conj(Q)) on object arrays."""
    PR = np.tensordot(P, R, axes=(1, 0))                            # [a, g, x]
    return np.transpose(np.tensordot(PR, _conj(Q), axes=(1, 1)), (0, 2, 1))       # [a, x, e] -> [a, e, x]


def _figure(x, W, S, f):
    d = x - f
    return mp.re(np.dot(_conj(d), np.dot(W, d))), np.dot(S, d)


def compute(cs):
    """The truth of one case: {field: fp64 / complex128 array}."""
    with mp.workdps(DIGITS):
        return _compute(cs)


def _compute(cs):
    B, N, n, m, d = cs.B, cs.N, cs.n, cs.m, cs.d
    gen = cs.kind == _lib.PLANT_GENERATOR
    cols = 1 if cs.kind == _lib.PLANT_HAMILTONIAN else d * d
    W = _lift(cs.W)
    S = W + _conj(W).T
    out = {"xs": np.empty((B, N + 1, n), dtype=complex), "q": np.empty((B, N + 1)), "J_sum": np.empty(B)}
    if not gen:
        out.update(U=np.empty((B, N, d, d), dtype=complex), dU=np.empty((B, N, m, d, d), dtype=complex),
                   grad_last=np.empty((B, N, m)), grad_sum=np.empty((B, N, m)), gs_last=np.empty((B, m)), gs_sum=np.empty((B, m)))
    for b in range(B):
        op0, ops = cs.member_ops(b)
        op0, ops = _lift(op0), [_lift(h) for h in ops]
        sc = [mp.mpf(float(s)) for s in cs.scale(b)]
        u = [[mp.mpf(float(x)) for x in row] for row in cs.useq(b)]
        f = _lift(cs.target(b))
        xs = [_lift(cs.x0[b])]
        Us, dUs = [], []
        for t in range(N):
            G = op0
            for k in range(m):
                G = G + ops[k] * (sc[k] * u[t][k])
            dt = mp.mpf(float(cs.dts[t]))
            if gen:
                xs.append(np.dot(_expm(G * dt), xs[-1]))
                continue
            fac = mp.mpc(0, -1) * dt
            X = G * fac
            U = _expm(X)
            zero = np.zeros((d, d), dtype=object) + mp.mpc(0)
            dUk = [_expm(np.block([[X, ops[k] * fac], [zero, X]]))[:d, d:] for k in range(m)]
            Us.append(U)
            dUs.append(dUk)
            xs.append(_sandwich(U, xs[-1].reshape(d, d, cols), U).reshape(-1))
            out["U"][b, t] = _cplx(U)
            out["dU"][b, t] = np.stack([_cplx(D) for D in dUk])
        qs, gts = zip(*[_figure(x, W, S, f) for x in xs])
        out["xs"][b] = np.stack([_cplx(x) for x in xs])
        out["q"][b] = [float(q) for q in qs]
        out["J_sum"][b] = float(mp.fsum(qs))
        if gen:
            continue
        for name, total in (("last", False), ("sum", True)):
            lam = gts[N]
            gs = [mp.mpf(0)] * m
            for t in range(N - 1, -1, -1):
                R = xs[t].reshape(d, d, cols)
                for k in range(m):
                    dx = (_sandwich(dUs[t][k], R, Us[t]) + _sandwich(Us[t], R, dUs[t][k])).reshape(-1)
                    ge = mp.re(np.dot(_conj(lam), dx))
                    out["grad_" + name][b, t, k] = float(sc[k] * ge)
                    gs[k] = gs[k] + u[t][k] * ge
                lam = _sandwich(_conj(Us[t]).T, lam.reshape(d, d, cols), _conj(Us[t]).T).reshape(-1)
                if total:
                    lam = lam + gts[t]
            out["gs_" + name][b] = [float(g) for g in gs]
    return out


def main():
    data = {}
    for key in sd.all_cases():
        cs = sd.case(*key)
        for field, a in compute(cs).items():
            data[cs.id + "/" + field] = a
        print(cs.id, flush=True)
    np.savez_compressed(sd.TRUTH_FILE, **data)
    print("wrote %s: %d arrays, %d bytes" % (sd.TRUTH_FILE, len(data), os.path.getsize(sd.TRUTH_FILE)))


if __name__ == "__main__":
    main()

"""Generate tests/golden/online_dmdc.npz: trajectories of small ensembles and what the REFERENCE's OnlineDMDc makes of them.

Run once where the reference checkout exists (its model.py is loaded by file path, as make_golden_dmdc_fit.py loads it; CPU only):
    python tests/golden/make_golden_online_dmdc.py
Per case the file holds data only: the inputs (xs [B, N + 1, n], us [N, m], u_scale [B, m], A0 [n, nz], alpha, discount, order) and,
from the reference's own OnlineDMDc.from_bootstrap(alpha=...) with .discount set, fed snapshot by snapshot through fit_iteration:
A after updates 5, 10, ... (A_hist [N // 5, B, n, nz]) and the final A and P.  (A and P after EVERY update of the nz = 64 case
alone would be 5 MB; every fifth A is what hist_every = 5 returns.)

The five cases are the (n, m, order, N, discount) of the issue that introduced the kernel, alpha = 1e2, one experiment:
  a (4, 1, 1, 12, 1.0), b (4, 1, 1, 12, 0.95): a driven, detuned qubit;  c (9, 2, 1, 40, 0.97): the three-level transmon;
  d (16, 3, 1, 40, 0.98): two coupled qubits under three drives;  e (16, 1, 1, 24, 0.95): the same under one drive.
The trajectories are held-control propagations of density matrices (make_golden_dmdc_fit.py's), two members per case with their
own plant parameters and drive calibration; A0 is the first-order model [I + dt L0 | dt L_k] of the nominal plant."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_dmdc_fit import I2, SX, SY, SZ, liou, load_reference, propagate, pulses, random_state, stacked  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
ALPHA = 1e2
EVERY = 5
B = 2


def euler_model(L0, Lk, dt):
    n = L0.shape[0]
    return np.hstack([np.identity(n) + dt * L0] + [dt * L for L in Lk])


def plant(name):
    """(drift(b, rng), control generators, dt, d, m) of a case."""
    if name in "ab":
        return (lambda b, rng: liou(0.5 * 0.05 * (b + 1) * SZ)), [liou(0.5 * SX)], 1.0, 2
    if name == "c":
        dt = 0.25
        alpha0 = -2 * np.pi * 0.1 / dt / 8
        a = np.diag(np.sqrt(np.arange(1, 3)), 1).astype(complex)
        P2 = np.zeros((3, 3), dtype=complex)
        P2[2, 2] = 1
        return ((lambda b, rng: liou((1 + 0.05 * rng.standard_normal()) * alpha0 * P2)),
                [liou(0.5 * (a.conj().T + a)), liou(0.5j * (a.conj().T - a))], dt, 3)
    Hk = [np.kron(SY, I2), np.kron(I2, SY), np.kron(SZ, I2)][:3 if name == "d" else 1]
    return (lambda b, rng: liou((1 + 0.02 * rng.standard_normal()) * np.kron(SZ, SZ))), [liou(h) for h in Hk], 0.25, 4


def make_case(ref, name, N, discount, rng):
    drift, Lk, dt, d = plant(name)
    m = len(Lk)
    us = pulses(rng, 1, N, m, 0.6 if d == 2 else 0.3)[0]
    u_scale = 1 + 0.02 * rng.standard_normal((B, m))
    x0 = random_state(rng, d)
    xs = np.stack([propagate(drift(b, rng), Lk, x0[None], (u_scale[b] * us)[None], dt)[0] for b in range(B)])
    nominal = drift(0, np.random.default_rng(0))
    A0 = euler_model(nominal, Lk, dt)
    n, nz = A0.shape
    A_hist = np.zeros((N // EVERY, B, n, nz), dtype=complex)
    A = np.zeros((B, n, nz), dtype=complex)
    P = np.zeros((B, nz, nz), dtype=complex)
    for b in range(B):
        X2, X1, UX1 = stacked(ref, xs[b][None], (u_scale[b] * us)[None], 1)
        model = ref["model"].OnlineDMDc.from_bootstrap(n, n, nz - n, A0.copy(), alpha=ALPHA)
        model.discount = discount
        for k in range(N):
            model.fit_iteration(X2[:, k], X1[:, k], UX1[:, k])
            if (k + 1) % EVERY == 0:
                A_hist[(k + 1) // EVERY - 1, b] = model.A
        A[b], P[b] = model.A, model.P
    print("%s: n = %d, nz = %d, N = %d, discount = %g; |A| up to %.3g, |P| up to %.3g, |A - A0| up to %.3g"
          % (name, n, nz, N, discount, np.abs(A).max(), np.abs(P).max(), np.abs(A - A0).max()))
    out = {"xs": xs, "us": us, "u_scale": u_scale, "A0": A0, "alpha": np.float64(ALPHA), "discount": np.float64(discount),
           "order": np.int64(1), "A_hist": A_hist, "A": A, "P": P}
    return {"%s_%s" % (name, k): v for k, v in out.items()}


def main():
    ref = load_reference()
    cases = {"a": (12, 1.0), "b": (12, 0.95), "c": (40, 0.97), "d": (40, 0.98), "e": (24, 0.95)}
    out = {}
    for i, (name, (N, discount)) in enumerate(cases.items()):
        out.update(make_case(ref, name, N, discount, np.random.default_rng([20240702, i])))
    path = os.path.join(OUT, "online_dmdc.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

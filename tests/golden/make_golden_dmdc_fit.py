"""Generate tests/golden/dmdc_fit.npz: training data of small ensembles and what the REFERENCE fits to them.

Run once where the reference checkout exists (it is loaded by file path, as make_golden.py loads it; CPU only):
    python tests/golden/make_golden_dmdc_fit.py
Per case the file holds the inputs (xs, us, u_scale, the chosen rconds) and, from the reference's own model.py / linearize.py,
A = DiscrepDMDc.from_data(X2, X1, krtimes(lift(U1), X1), rcond=rcond).A per member and rcond, the singular values of the stacked
data Z = [X1; UX1], the rank numpy's pinv keeps, and `sens`: how far the reference's own A moves when the data are perturbed by a
relative 1e-15 (the floor below which no other route to A can be told from it).  The trajectories are made here with
scipy.linalg.expm (exact held-control propagators) or, for the bilinear case, by iterating a random stable model.

Each case's rconds are taken from the reference's training grid np.logspace(-6, -1, 10) such that (asserted)
  - every cut-off rcond s_0 is at least a factor MARGIN = 1.2 away from every singular value of every member, and
  - at least two different ranks occur in the case,
so that no member's rank hangs on rounding: a Gram eigenvalue moves by eps (s_0 / s_i)^2 relative, far inside that margin."""
import importlib.util
import math
import os
import sys
import types

import numpy as np
from scipy.linalg import expm

REF = "/root/reference/mpc4quantum/"
OUT = os.path.dirname(os.path.abspath(__file__))
GRID = np.logspace(-6, -1, 10)
MARGIN = 1.2

SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]], dtype=complex)
SZ = np.array([[1, 0], [0, -1]], dtype=complex)
I2 = np.identity(2, dtype=complex)


def load_reference():
    np.product = np.prod
    np.math = math
    pkg = types.ModuleType("m4q_reference")
    pkg.__path__ = [REF]
    sys.modules["m4q_reference"] = pkg
    sys.modules.setdefault("qutip", types.ModuleType("qutip"))
    mods = {}
    for name in ("linearize", "model"):
        spec = importlib.util.spec_from_file_location("m4q_reference." + name, REF + name + ".py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules["m4q_reference." + name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def liou(H):
    d = H.shape[0]
    return -1j * (np.kron(H, np.identity(d)) - np.kron(np.identity(d), H.T))


def random_state(rng, d, mix=0.3):
    """A full-rank density matrix, row-major vectorised."""
    a = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    rho = a @ a.conj().T
    rho = (1 - mix) * rho / np.trace(rho).real + mix * np.identity(d) / d
    return rho.reshape(-1)


def pulses(rng, E, N, m, amp):
    """Smooth pulses: a Gaussian envelope per control with its own centre, width and carrier, [E, N, m]."""
    t = np.arange(N)[None, :, None]
    centre = rng.uniform(0.25, 0.75, (E, 1, m)) * N
    width = rng.uniform(0.15, 0.35, (E, 1, m)) * N
    phase = rng.uniform(0, 2 * np.pi, (E, 1, m))
    freq = rng.uniform(0.0, 0.4, (E, 1, m))
    return amp * np.exp(-0.5 * ((t - centre) / width) ** 2) * np.cos(freq * t + phase)


def propagate(gens0, gensk, x0, u, dt):
    """x_{t+1} = expm(dt (L0 + sum_k u_t[k] L_k)) x_t; x0 [E, n], u [E, N, m] -> [E, N + 1, n]."""
    E, N, m = u.shape
    xs = np.zeros((E, N + 1, x0.shape[1]), dtype=complex)
    xs[:, 0] = x0
    for e in range(E):
        for t in range(N):
            L = gens0 + sum(u[e, t, k] * gensk[k] for k in range(m))
            xs[e, t + 1] = expm(dt * L) @ xs[e, t]
    return xs


def case_qubit(rng, order, B, E, N, amp, resonant=False):
    """A driven qubit from its ground state, one detuning and drive strength per member.  resonant: no detuning - the Bloch vector
    stays in one plane, so the stacked data have rank 3 (1 + P) of 4 (1 + P) and truncation decides the answer."""
    xs, dt = [], 1.0
    u = pulses(rng, E, N, 1, amp)
    rho0 = np.array([1, 0, 0, 0], dtype=complex)
    for b in range(B):
        delta = 0.0 if resonant else 0.05 * (b + 1)
        xs.append(propagate(liou(0.5 * delta * SZ), [liou(0.5 * (1 + 0.1 * b) * SX)], np.tile(rho0, (E, 1)), u, dt))
    return dict(xs=np.stack(xs), us=u, order=order)


def case_transmon(rng, B, E, N):
    """The three-level transmon of the flagship configuration with per-member detuning and drive calibration (u_scale)."""
    dt = 0.25
    alpha0 = -2 * np.pi * 0.1 / dt / 8
    a = np.diag(np.sqrt(np.arange(1, 3)), 1).astype(complex)
    HX, HY = 0.5 * (a.conj().T + a), 0.5j * (a.conj().T - a)
    P2 = np.zeros((3, 3), dtype=complex)
    P2[2, 2] = 1
    u = pulses(rng, E, N, 2, 0.3)
    u_scale = 1 + 0.02 * rng.standard_normal((B, 2))
    x0 = np.stack([random_state(rng, 3) for _ in range(E)])
    xs = []
    for b in range(B):
        drift = (1 + 0.05 * rng.standard_normal()) * alpha0
        xs.append(propagate(liou(drift * P2), [liou(HX), liou(HY)], x0, u_scale[b] * u, dt))
    return dict(xs=np.stack(xs), us=u, u_scale=u_scale, order=1)


def case_bilinear(rng, B, E, N, n=8, m=2):
    """A random stable bilinear model x+ = A x + sum_k u_k N_k x on a state space that is no square (two reduced qubit states),
    its own controls per member."""
    xs, us = [], []
    for b in range(B):
        A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        A *= 0.95 / np.abs(np.linalg.eigvals(A)).max()
        Nk = 0.3 * (rng.standard_normal((m, n, n)) + 1j * rng.standard_normal((m, n, n))) / np.sqrt(n)
        u = 0.3 * rng.uniform(-1, 1, (E, N, m))
        x = np.zeros((E, N + 1, n), dtype=complex)
        x[:, 0] = rng.standard_normal((E, n)) + 1j * rng.standard_normal((E, n))
        for e in range(E):
            for t in range(N):
                x[e, t + 1] = A @ x[e, t] + sum(u[e, t, k] * (Nk[k] @ x[e, t]) for k in range(m))
        xs.append(x)
        us.append(u)
    return dict(xs=np.stack(xs), us=np.stack(us), order=1)


def case_two_qubits(rng, B, E, N):
    """Two coupled qubits under three drives (n = 16, nz = 64), the coupling per member."""
    dt = 0.25
    Hk = [np.kron(SY, I2), np.kron(I2, SY), np.kron(SZ, I2)]
    u = pulses(rng, E, N, 3, 0.3)
    x0 = np.stack([random_state(rng, 4) for _ in range(E)])
    xs = []
    for b in range(B):
        J = 1 + 0.02 * rng.standard_normal()
        xs.append(propagate(liou(J * np.kron(SZ, SZ)), [liou(h) for h in Hk], x0, u, dt))
    return dict(xs=np.stack(xs), us=u, order=1)


def stacked(ref, xs_b, u_b, order):
    """X2, X1, UX1 of one member as the reference's training workflow stacks them (experiments side by side)."""
    lin = ref["linearize"]
    fns = lin.create_library(order, u_b.shape[-1])[1:]
    X2, X1, UX1 = [], [], []
    for e in range(xs_b.shape[0]):
        x = xs_b[e].T                                   # (n, N + 1)
        U1 = np.vstack([f(u_b[e].T) for f in fns])      # (P, N)
        X2.append(x[:, 1:])
        X1.append(x[:, :-1])
        UX1.append(lin.krtimes(U1, x[:, :-1]))
    return np.hstack(X2), np.hstack(X1), np.hstack(UX1)


def spectrum(ref, case):
    """Per member the stacked data (X2, X1, UX1) and the singular values of Z = [X1; UX1]."""
    xs, us, order = case["xs"], case["us"], case["order"]
    u_scale = case.get("u_scale")
    data, svals = [], []
    for b in range(xs.shape[0]):
        u_b = us[b] if us.ndim == 4 else us
        if u_scale is not None:
            u_b = u_scale[b] * u_b
        X2, X1, UX1 = stacked(ref, xs[b], u_b, order)
        data.append((X2, X1, UX1))
        svals.append(np.linalg.svd(np.vstack([X1, UX1]), compute_uv=False))
    return data, np.stack(svals)


def choose_rconds(svals):
    """The grid points whose cut-off stays clear of every singular value of every member, and the ranks they give [R, B].
    (Singular values at the rounding floor of the SVD, 1e-16 s_0, are far under every cut-off of the grid.)"""
    ok = []
    for rc in GRID:
        ratio = svals / (rc * svals[:, :1])
        if np.all((ratio >= MARGIN) | (ratio <= 1 / MARGIN)):
            ok.append(rc)
    rconds = np.array(ok)
    rank = np.stack([(svals > rc * svals[:, :1]).sum(axis=1) for rc in rconds]) if ok else np.zeros((0, svals.shape[0]), int)
    if len(rconds) > 4:          # keep four cut-offs, the extreme ranks among them
        by_rank = np.argsort(rank.sum(axis=1), kind="stable")
        pick = sorted({by_rank[0], by_rank[-1], by_rank[len(by_rank) // 3], by_rank[2 * len(by_rank) // 3]})
        rconds, rank = rconds[pick], rank[pick]
    return rconds, rank


def record(ref, name, case, rng):
    xs, us, order = case["xs"], case["us"], case["order"]
    u_scale = case.get("u_scale")
    B = xs.shape[0]
    data, svals = spectrum(ref, case)
    nz = data[0][1].shape[0] + data[0][2].shape[0]
    assert svals.shape[1] == nz, "fewer snapshots than rows"
    rconds, rank = choose_rconds(svals)
    for rc in rconds:
        ratio = svals / (rc * svals[:, :1])
        assert np.all((ratio >= MARGIN) | (ratio <= 1 / MARGIN))
    assert len(np.unique(rank)) >= 2, "%s: the admissible cut-offs %s give ranks %s" % (name, rconds, np.unique(rank))
    Model = ref["model"].DiscrepDMDc
    n = xs.shape[-1]
    A = np.zeros((len(rconds), B, n, nz), dtype=complex)
    sens = np.zeros((len(rconds), B))
    for b, (X2, X1, UX1) in enumerate(data):
        def jitter(M):
            return M * (1 + 1e-15 * rng.standard_normal(M.shape))
        pert = (jitter(X2), jitter(X1), jitter(UX1))
        for r, rc in enumerate(rconds):
            A[r, b] = Model.from_data(X2, X1, UX1, rcond=rc).A
            assert np.linalg.matrix_rank(np.vstack([X1, UX1]), tol=rc * svals[b, 0]) == rank[r, b]
            sens[r, b] = np.abs(Model.from_data(*pert, rcond=rc).A - A[r, b]).max()
    out = {"xs": xs, "us": us, "order": np.int64(order), "rconds": rconds, "A": A, "svals": svals, "rank": rank.astype(np.int32),
           "sens": sens}
    if u_scale is not None:
        out["u_scale"] = u_scale
    kappa = svals[:, :1] / np.stack([svals[np.arange(B), rank[r] - 1] for r in range(len(rconds))]).T
    print("%s: n = %d, nz = %d, B = %d, E = %d, N = %d; rconds %s; ranks %s; kappa up to %.3g; sens up to %.3g; |A| up to %.3g"
          % (name, n, nz, B, xs.shape[1], xs.shape[2] - 1, rconds, [sorted(set(r)) for r in rank.tolist()], kappa.max(),
             sens.max(), np.abs(A).max()))
    return {"%s_%s" % (name, k): v for k, v in out.items()}


def main():
    """Every case draws its data from its own seed sequence; a draw none of whose admissible cut-offs truncates (dense spectra
    leave few grid points clear of all singular values) is passed over for the next one, so the file is reproducible."""
    ref = load_reference()
    builders = {
        "a": lambda rng: case_qubit(rng, 1, B=3, E=1, N=12, amp=0.6, resonant=True),
        "b": lambda rng: case_transmon(rng, B=5, E=3, N=40),
        "c": lambda rng: case_qubit(rng, 2, B=3, E=2, N=20, amp=0.8),
        "d": lambda rng: case_bilinear(rng, B=3, E=4, N=16),
        "e": lambda rng: case_two_qubits(rng, B=2, E=4, N=40),
    }
    out = {}
    for i, (name, make) in enumerate(builders.items()):
        for attempt in range(200):
            rng = np.random.default_rng([20240611, i, attempt])
            case = make(rng)
            if len(np.unique(choose_rconds(spectrum(ref, case)[1])[1])) >= 2:
                break
        print("case %s: draw %d" % (name, attempt))
        out.update(record(ref, name, case, rng))
    path = os.path.join(OUT, "dmdc_fit.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

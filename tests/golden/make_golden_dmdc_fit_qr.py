"""Generate tests/golden/dmdc_fit_qr.npz: ill-conditioned training data of small ensembles and what the REFERENCE fits to them,
for the QR route of the batched fit (m4q_dmdc_fit_qr_batch, mpc4quantum_amd/fit.py: dmdc_fit_qr_reference).

Run once where the reference checkout exists (its model.py is loaded by file path, as make_golden_dmdc_fit.py loads it; CPU only):
    python tests/golden/make_golden_dmdc_fit_qr.py
Four cases of two members each, every member with its own detuning (or coupling) and drive calibration u_scale, N = 40 steps:
  p (4, 1, 1), nz = 8: a driven, detuned qubit, one pulse;
  q (9, 2, 1), nz = 27: the three-level transmon of the flagship configuration, ONE experiment with one Gaussian pulse per drive
    at the configuration's saturation amplitude - noise-free data whose singular values fall steadily to the rounding floor;
  r (9, 2, 2), nz = 54: the same plant under four such experiments, second-order library;
  s (16, 3, 1), nz = 64: two coupled qubits under three drives, four experiments (every lane of the wavefront busy).
Per case the file holds data only: xs, us, u_scale, order, the chosen rconds and, from the reference's own model.py,
A = DiscrepDMDc.from_data(X2, X1, krtimes(lift(U1), X1), rcond).A per cut-off and member, the singular values of the stacked data,
the rank numpy's pinv keeps, and sens [R][B]: how far the reference's own A moves (max |dA|) when xs and us are perturbed by a
relative 1e-15, the largest of three draws.

The cut-offs come from GRID = np.logspace(-10, -1, 37) (quarter decades) such that (asserted here, and again by
tests/test_fit_qr_host.py from the file)
  - every cut-off rcond s_0 is a factor MARGIN = 1.2 away from every singular value of both members,
  - sens <= 1e-8 max(1, |A|_inf) for both members (a cut-off at which the reference itself is less certain is passed over),
  - at least two ranks occur in the case, cases q and s hold a cut-off <= 1e-8,
  - the definition (mpc4quantum_amd.fit.dmdc_fit_qr_reference) converges on both members within SWEEPS_MAX = 18 sweeps, so that
    the 20 the host test allows and the cap of 30 are never why a case passes, and
  - over the file the cut-offs reach from 1e-10 to 1e-1 and some (case, rcond) has kappa_r = s_0 / s_rank >= 1e5."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mpc4quantum_amd.fit import dmdc_fit_qr_reference  # noqa: E402
from make_golden_dmdc_fit import I2, MARGIN, SX, SY, SZ, liou, load_reference, propagate, random_state, stacked  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
GRID = np.logspace(-10, -1, 37)
B, N = 2, 40
SAT = 2 * np.pi * 0.25                      # the flagship configuration's control bound
SENS_MAX = 1e-8
KEEP = 5                                    # cut-offs kept per case
SWEEPS_MAX = 18


def gaussian_pulses(rng, E, m, amp):
    """One Gaussian pulse per experiment and control, peak `amp`, its own centre and width: [E, N, m]."""
    t = np.arange(N)[None, :, None]
    centre = rng.uniform(0.3, 0.7, (E, 1, m)) * N
    width = rng.uniform(0.12, 0.3, (E, 1, m)) * N
    return amp * np.exp(-0.5 * ((t - centre) / width) ** 2)


def case_qubit(rng):
    us = gaussian_pulses(rng, 1, 1, 0.6)
    u_scale = 1 + 0.02 * rng.standard_normal((B, 1))
    x0 = random_state(rng, 2)[None]
    xs = [propagate(liou(0.5 * 0.05 * (b + 1) * SZ), [liou(0.5 * SX)], x0, u_scale[b] * us, 1.0) for b in range(B)]
    return dict(xs=np.stack(xs), us=us, u_scale=u_scale, order=1)


def case_transmon(rng, order, E):
    dt = 0.25
    alpha0 = -2 * np.pi * 0.1 / dt / 8
    a = np.diag(np.sqrt(np.arange(1, 3)), 1).astype(complex)
    HX, HY = 0.5 * (a.conj().T + a), 0.5j * (a.conj().T - a)
    P2 = np.zeros((3, 3), dtype=complex)
    P2[2, 2] = 1
    us = gaussian_pulses(rng, E, 2, SAT)
    u_scale = 1 + 0.02 * rng.standard_normal((B, 2))
    x0 = np.stack([random_state(rng, 3) for _ in range(E)])
    xs = []
    for b in range(B):
        drift = (1 + 0.05 * rng.standard_normal()) * alpha0
        xs.append(propagate(liou(drift * P2), [liou(HX), liou(HY)], x0, u_scale[b] * us, dt))
    return dict(xs=np.stack(xs), us=us, u_scale=u_scale, order=order)


def case_two_qubits(rng, E):
    Hk = [np.kron(SY, I2), np.kron(I2, SY), np.kron(SZ, I2)]
    us = gaussian_pulses(rng, E, 3, 0.3)
    u_scale = 1 + 0.02 * rng.standard_normal((B, 3))
    x0 = np.stack([random_state(rng, 4) for _ in range(E)])
    xs = []
    for b in range(B):
        J = 1 + 0.02 * rng.standard_normal()
        xs.append(propagate(liou(J * np.kron(SZ, SZ)), [liou(h) for h in Hk], x0, u_scale[b] * us, 0.25))
    return dict(xs=np.stack(xs), us=us, u_scale=u_scale, order=1)


def fits(ref, case, xs, us, rconds):
    """The reference's A [R, B, n, nz] for data (xs, us) of the case's shape, and the singular values of the stacked data [B, nz]."""
    Model = ref["model"].DiscrepDMDc
    A, svals = [], []
    for b in range(B):
        X2, X1, UX1 = stacked(ref, xs[b], case["u_scale"][b] * us, case["order"])
        svals.append(np.linalg.svd(np.vstack([X1, UX1]), compute_uv=False))
        A.append([Model.from_data(X2, X1, UX1, rcond=rc).A for rc in rconds])
    return np.array(A).transpose(1, 0, 2, 3), np.stack(svals)


def clear_of_spectrum(svals, rconds):
    ratio = svals[None] / (rconds[:, None, None] * svals[None, :, :1])
    return np.all((ratio >= MARGIN) | (ratio <= 1 / MARGIN), axis=(1, 2))


def record(ref, name, case, rng):
    xs, us = case["xs"], case["us"]
    A, svals = fits(ref, case, xs, us, GRID)
    assert svals.shape[1] == A.shape[3], "fewer snapshots than rows"
    sens = np.zeros(A.shape[:2])
    for _ in range(3):
        moved, _ = fits(ref, case, xs * (1 + 1e-15 * rng.standard_normal(xs.shape)), us * (1 + 1e-15 * rng.standard_normal(us.shape)),
                        GRID)
        sens = np.maximum(sens, np.abs(moved - A).max(axis=(2, 3)))
    scale = np.maximum(1.0, np.abs(A).max(axis=(2, 3)))
    ok = clear_of_spectrum(svals, GRID) & np.all(sens <= SENS_MAX * scale, axis=1)
    rank = (svals[None] > GRID[:, None, None] * svals[None, :, :1]).sum(axis=2)                  # [grid, B]
    idx = np.nonzero(ok)[0]
    if len(idx):
        # kept: the lowest admissible cut-off of every rank and the highest of all, thinned evenly to KEEP, and with them the
        # lowest one that the Gram route accepts too (>= 1e-7), where the two routes meet at the worst conditioning
        first = [i for k, i in enumerate(idx) if k == 0 or not np.array_equal(rank[i], rank[idx[k - 1]])]
        gram = [i for i in idx if GRID[i] >= 1e-7 * (1 - 1e-12)][:1]
        some = np.unique(first + [idx[-1]])
        idx = np.unique(list(some[np.unique(np.round(np.linspace(0, len(some) - 1, KEEP - 1)).astype(int))]) + gram)
    rconds, A, sens, rank = GRID[idx], A[idx], sens[idx], rank[idx].astype(np.int32)
    kappa = svals[None, :, 0] / svals[np.arange(B)[None, :], rank - 1]
    summary = ("%s: n = %d, nz = %d, E = %d; rconds %s; ranks %s; kappa_r %s; sens up to %.3g; |A| up to %.3g"
               % (name, xs.shape[-1], A.shape[3], xs.shape[1], rconds, rank.tolist(), np.array2string(kappa, precision=2),
                  sens.max() if len(idx) else 0, np.abs(A).max() if len(idx) else 0))
    good = len(idx) >= 2 and len(np.unique(rank)) >= 2 and (name not in "qs" or rconds.min() <= 1e-8)
    if good:
        sweeps = dmdc_fit_qr_reference(xs, us, case["order"], rconds, case["u_scale"])["sweeps"]
        summary += "; sweeps %s" % sweeps
        good = bool(np.all(sweeps <= SWEEPS_MAX))
    out = {"xs": xs, "us": us, "u_scale": case["u_scale"], "order": np.int64(case["order"]), "rconds": rconds, "A": A, "svals": svals,
           "rank": rank, "sens": sens}
    return good, summary, kappa, {"%s_%s" % (name, k): v for k, v in out.items()}


def main():
    """Every case draws its data from its own seed sequence; a draw whose admissible cut-offs do not meet the case's conditions
    is passed over for the next one, so the file is reproducible."""
    ref = load_reference()
    builders = {"p": case_qubit, "q": lambda rng: case_transmon(rng, 1, 1), "r": lambda rng: case_transmon(rng, 2, 4),
                "s": lambda rng: case_two_qubits(rng, 4)}
    out, kappas, lo, hi = {}, [], 1.0, 0.0
    for i, (name, make) in enumerate(builders.items()):
        for attempt in range(50):
            rng = np.random.default_rng([20240815, i, attempt])
            good, summary, kappa, arrays = record(ref, name, make(rng), rng)
            if good:
                break
            print("passed over: draw %d  %s" % (attempt, summary))
        assert good, "case %s: no admissible draw" % name
        print("draw %d  %s" % (attempt, summary))
        out.update(arrays)
        kappas.append(kappa.max())
        lo, hi = min(lo, arrays[name + "_rconds"].min()), max(hi, arrays[name + "_rconds"].max())
    assert lo <= 1e-10 * (1 + 1e-12) and hi >= 1e-1 * (1 - 1e-12), (lo, hi)
    assert max(kappas) >= 1e5, kappas
    path = os.path.join(OUT, "dmdc_fit_qr.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The batched recursive DMDc update on the device against the host loop it replaces.

    python tools/online_bench.py [--members 65536] [--host-members 1024] [--repeats 3] [--once] [--hermitian]

Config 3's plant (the three-level transmon under two drives), `members` of them with per-member detuning (op0 scaled) and drive
calibration (u_scale), one trajectory of N = 40 held-control steps per member from plant_rollout_batch under one smooth pulse pair
shared by the ensemble.  Every member's model starts from the nominal first-order model (one A0 for the ensemble), P0 = 1e2 I,
discount 0.97, and takes its 40 snapshots in ONE m4q_online_dmdc_batch call.
Printed: the wall time of that call (host buffers in and out, as the one-shot entry points copy them) per repeat, the host loop
OnlineDMDc.fit_iteration timed on the first `host-members` members and scaled to the ensemble, and the largest difference
between the two on those members relative to max |A| / max |P|.  No threshold is set: nothing upstream updates an ensemble.
--once runs the device call exactly once and times nothing: the run to put under `rocprofv3 --kernel-trace --stats`, a run of its
own, whose kernel statistics give online_dmdc_kernel's time without the copies."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q                       # noqa: E402
from mpc4quantum_amd import configs, fit            # noqa: E402

N, ALPHA, DISCOUNT = 40, 1e2, 0.97


def run_data(B):
    p = configs.build(3, batch=B, host_models=False, drift_scale=0.125)
    rng = np.random.default_rng(13)
    op0 = np.ascontiguousarray(p["scales"][:, 0, None, None] * p["plant_op0"])
    u_scale = np.ascontiguousarray(p["scales"][:, 1:])
    t = np.arange(N)[:, None]
    us = 0.3 * np.exp(-0.5 * ((t - rng.uniform(10, 30, (1, 2))) / rng.uniform(6, 14, (1, 2))) ** 2) \
        * np.cos(rng.uniform(0, 0.4, (1, 2)) * t + rng.uniform(0, 2 * np.pi, (1, 2)))
    a = rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3))
    rho = a @ a.conj().T
    rho = 0.7 * rho / np.trace(rho).real + 0.1 * np.identity(3)
    xs = m4q.plant_rollout_batch(np.tile(rho.reshape(1, -1), (B, 1)), us, op0, p["plant_ops"][0], p["dt"], u_scale=u_scale)["xs"]
    A0 = m4q.discretize_homogeneous(list(p["generators"]), p["dt"], 1)
    return np.ascontiguousarray(xs), us, u_scale, np.ascontiguousarray(A0, dtype=complex)


def host_loop(xs, us, u_scale, A0):
    B, n = xs.shape[0], xs.shape[-1]
    nz = A0.shape[1]
    A = np.empty((B, n, nz), dtype=complex)
    P = np.empty((B, nz, nz), dtype=complex)
    for b in range(B):
        Z, Y = fit.stack_snapshots(xs[b][None], (u_scale[b] * us)[None], 1)
        model = m4q.OnlineDMDc.from_bootstrap(n, n, nz - n, A0.copy(), alpha=ALPHA)
        model.discount = DISCOUNT
        for k in range(Z.shape[1]):
            model.fit_iteration(Y[:, k], Z[:n, k], Z[n:, k])
        A[b], P[b] = model.A, model.P
    return A, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--host-members", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--hermitian", action="store_true")
    a = ap.parse_args()
    B, Bh = a.members, min(a.host_members, a.members)
    xs, us, u_scale, A0 = run_data(B)
    kw = dict(alpha=ALPHA, discount=DISCOUNT, u_scale=u_scale, hermitian=a.hermitian)
    out = m4q.online_dmdc_batch(xs, us, 1, A0, **kw)                          # warm-up (and, with --once, the only run)
    print("online_bench B=%d n=9 m=2 nz=27 N=%d discount=%g alpha=%g%s: status counts %s" %
          (B, N, DISCOUNT, ALPHA, " hermitian" if a.hermitian else "", np.bincount(out["status"], minlength=4).tolist()), flush=True)
    print("online_bench PCIe bytes: %.4g MB in, %.4g MB out" %
          ((xs.nbytes + us.nbytes + u_scale.nbytes + A0.nbytes) / 1e6, (out["models"].nbytes + out["P"].nbytes) / 1e6), flush=True)
    if a.once:
        return
    for r in range(a.repeats):
        t0 = time.perf_counter()
        m4q.online_dmdc_batch(xs, us, 1, A0, **kw)
        dt = time.perf_counter() - t0
        print("online_bench repeat %d device call wall %9.2f ms  %.3e updates/s (%d members x %d snapshots)" %
              (r, 1e3 * dt, B * N / dt, B, N), flush=True)
    if a.hermitian:
        return                                                                # (the host class has the plain form only)
    t0 = time.perf_counter()
    A, P = host_loop(xs[:Bh], us, u_scale[:Bh], A0)
    dt = time.perf_counter() - t0
    print("online_bench host loop OnlineDMDc.fit_iteration: %d members %.2f ms, scaled to %d members %.2f ms" %
          (Bh, 1e3 * dt, B, 1e3 * dt * B / Bh), flush=True)
    eA = (np.abs(out["models"][:Bh] - A).max(axis=(1, 2)) / np.abs(A).max(axis=(1, 2))).max()
    eP = (np.abs(out["P"][:Bh] - P).max(axis=(1, 2)) / np.abs(P).max(axis=(1, 2))).max()
    print("online_bench device against host on %d members: max |A - A_host| / max |A| %.3e, max |P - P_host| / max |P| %.3e" %
          (Bh, eA, eP), flush=True)


if __name__ == "__main__":
    main()

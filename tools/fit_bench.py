#!/usr/bin/env python3
"""The batched DMDc fit on the device against the host loop it replaces.

    python tools/fit_bench.py [--method gram|qr] [--members 65536] [--host-members 1024] [--repeats 3] [--once]
    python tools/fit_bench.py --prior [--members 65536] [--repeats 5] [--cutoffs 10]

Config 3's plant (the three-level transmon under two drives), `members` of them with per-member detuning (op0 scaled) and drive
calibration (u_scale), E = 3 training experiments of N = 40 held-control steps from random full-rank states, one smooth pulse set
shared by the ensemble; the trajectories come from plant_rollout_batch (one launch per experiment).  Fitted for the ten rconds of
the reference's training grid np.logspace(-6, -1, 10) in ONE m4q_dmdc_fit_batch call, or - with --method qr - in one
m4q_dmdc_fit_qr_batch call on the same inputs (the time to hold it against is --method gram's; accuracy is the point of the QR
route, so no threshold is set there either).
Printed: the wall time of that call (host buffers in and out, as the one-shot entry points copy them: 2.5 GB of models come back
at 65,536 members) per repeat, the host loop `DiscrepDMDc.from_data` over the same rconds timed on the first `host-members`
members and scaled to the ensemble, and the largest difference between the two on those members at the cut-offs where their ranks
agree.  No threshold is set: nothing upstream fits an ensemble.
--once runs the device fit exactly once and times nothing: the run to put under `rocprofv3 --kernel-trace --stats`, a run of its
own, whose kernel statistics give dmdc_fit_kernel's (dmdc_fit_qr_kernel's) time without the copies.
--prior times the fit against a prior model (m4q_dmdc_refit_batch / m4q_dmdc_refit_qr_batch: A0 = the nominal model of the ensemble
from m4q_discretize_batch, discount 0.98, full counts) against the plain fit of the same build on the same inputs, both routes: after
one warm-up call of each of the four entry points the calls alternate plain, prior, plain, ... `repeats` times; the medians of the
wall times and their ratio are printed per route.  --cutoffs K fits the first K points of the grid: with one, the 2.5 GB of models
that ten cut-offs copy back no longer hide the kernels."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q                       # noqa: E402
from mpc4quantum_amd import configs, fit            # noqa: E402

E, N = 3, 40
RCONDS = np.logspace(-6, -1, 10)


def training_data(B):
    p = configs.build(3, batch=B, host_models=False, drift_scale=0.125)
    rng = np.random.default_rng(12)
    op0 = np.ascontiguousarray(p["scales"][:, 0, None, None] * p["plant_op0"])
    u_scale = np.ascontiguousarray(p["scales"][:, 1:])
    t = np.arange(N)[None, :, None]
    us = 0.3 * np.exp(-0.5 * ((t - rng.uniform(10, 30, (E, 1, 2))) / rng.uniform(6, 14, (E, 1, 2))) ** 2) \
        * np.cos(rng.uniform(0, 0.4, (E, 1, 2)) * t + rng.uniform(0, 2 * np.pi, (E, 1, 2)))
    xs = np.empty((B, E, N + 1, 9), dtype=complex)
    for e in range(E):
        a = rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3))
        rho = a @ a.conj().T
        rho = 0.7 * rho / np.trace(rho).real + 0.1 * np.identity(3)
        x0 = np.tile(rho.reshape(1, -1), (B, 1))
        xs[:, e] = m4q.plant_rollout_batch(x0, us[e], op0, p["plant_ops"][0], p["dt"], u_scale=u_scale)["xs"]
    return xs, us, u_scale


def host_fit(xs, us, u_scale):
    B, n = xs.shape[0], xs.shape[-1]
    out = np.empty((len(RCONDS), B, n, 3 * n), dtype=complex)
    for b in range(B):
        Z, Y = fit.stack_snapshots(xs[b], u_scale[b] * us, 1)
        for r, rc in enumerate(RCONDS):
            out[r, b] = m4q.DiscrepDMDc.from_data(Y, Z[:n], Z[n:], rcond=rc).A
    return out


def prior_bench(B, repeats, cutoffs):
    xs, us, u_scale = training_data(B)
    p = configs.build(3, batch=1, host_models=False, drift_scale=0.125)
    A0 = m4q.discretize_homogeneous_batch(list(p["generators"]), p["dt"], 1)[0]
    rconds = RCONDS[:cutoffs]
    for method in fit.METHODS:
        calls = {"plain": lambda: m4q.dmdc_fit_batch(xs, us, 1, rconds, u_scale=u_scale, method=method),
                 "prior": lambda: m4q.dmdc_fit_batch(xs, us, 1, rconds, u_scale=u_scale, method=method, A0=A0, discount=0.98)}
        warm = {k: f() for k, f in calls.items()}
        print("fit_bench --prior method=%s B=%d n=9 m=2 E=%d N=%d R=%d: status counts plain %s prior %s, max |A_prior - A_plain| %.3g"
              % (method, B, E, N, len(rconds), np.bincount(warm["plain"]["status"], minlength=4).tolist(),
                 np.bincount(warm["prior"]["status"], minlength=4).tolist(), np.abs(warm["prior"]["models"] - warm["plain"]["models"]).max()),
              flush=True)
        del warm
        times = {k: [] for k in calls}
        for r in range(repeats):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                times[k].append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) for k, v in times.items()}
        for k in calls:
            print("fit_bench --prior method=%s %s call wall ms: %s  median %.2f" %
                  (method, k, " ".join("%.2f" % (1e3 * t) for t in times[k]), 1e3 * med[k]), flush=True)
        print("fit_bench --prior method=%s median prior / median plain = %.3f" % (method, med["prior"] / med["plain"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", choices=fit.METHODS, default="gram")
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--host-members", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--prior", action="store_true")
    ap.add_argument("--cutoffs", type=int, default=len(RCONDS))
    a = ap.parse_args()
    if a.prior:
        return prior_bench(a.members, max(a.repeats, 5), max(1, min(a.cutoffs, len(RCONDS))))
    B, Bh = a.members, min(a.host_members, a.members)
    xs, us, u_scale = training_data(B)
    out = m4q.dmdc_fit_batch(xs, us, 1, RCONDS, u_scale=u_scale, method=a.method)   # warm-up (and, with --once, the only run)
    print("fit_bench method=%s B=%d n=9 m=2 E=%d N=%d R=%d: status counts %s, ranks per rcond (member 0) %s" %
          (a.method, B, E, N, len(RCONDS), np.bincount(out["status"], minlength=4).tolist(), out["rank"][:, 0].tolist()), flush=True)
    print("fit_bench PCIe bytes: %.4g MB in, %.4g MB out" %
          ((xs.nbytes + us.nbytes + u_scale.nbytes) / 1e6, (out["models"].nbytes + out["rank"].nbytes + out["svals"].nbytes) / 1e6), flush=True)
    if a.once:
        return
    for r in range(a.repeats):
        t0 = time.perf_counter()
        m4q.dmdc_fit_batch(xs, us, 1, RCONDS, u_scale=u_scale, method=a.method)
        dt = time.perf_counter() - t0
        print("fit_bench repeat %d device call wall %9.2f ms  %.3e fits/s (%d members x %d rconds)" %
              (r, 1e3 * dt, B * len(RCONDS) / dt, B, len(RCONDS)), flush=True)
    t0 = time.perf_counter()
    host = host_fit(xs[:Bh], us, u_scale[:Bh])
    dt = time.perf_counter() - t0
    print("fit_bench host loop DiscrepDMDc.from_data: %d members %.2f ms, scaled to %d members %.2f ms" %
          (Bh, 1e3 * dt, B, 1e3 * dt * B / Bh), flush=True)
    Zs = [np.linalg.svd(fit.stack_snapshots(xs[b], u_scale[b] * us, 1)[0], compute_uv=False) for b in range(Bh)]
    host_rank = np.array([[int((s > rc * s[0]).sum()) for s in Zs] for rc in RCONDS])
    same = host_rank == out["rank"][:, :Bh]
    diff = np.abs(out["models"][:, :Bh] - host).max(axis=(2, 3))
    print("fit_bench device against host on %d members: ranks agree on %d of %d fits, max |A - A_host| there %.3e" %
          (Bh, int(same.sum()), same.size, diff[same].max()), flush=True)


if __name__ == "__main__":
    main()

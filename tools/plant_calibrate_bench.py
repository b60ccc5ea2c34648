#!/usr/bin/env python3
"""The plant-parameter gradient of an ensemble against the control gradient, and the calibration that runs on it (DESIGN.md
section 5.17).

    python tools/plant_calibrate_bench.py [--repeats 3] [--members 65536] [--steps 20] [--iters 40] [--sigma 1e-3]

Config 3's plant (the DRAG transmon, (dim_x, dim_u) = (9, 2)), 65,536 members whose detuning and anharmonicity (p = 2: the number
operator and n (n - 1) / 2) are drawn within +-0.2 of the nominal scales around the nominal drift, N steps of one seeded pulse
shared by the ensemble.  The data are plant_rollout_batch's trajectories of the true plants, as they are and with
MeasurementNoise(sigma, kind="hermitian") added to every measured column.
Two gradient variants on the same ensemble, alternated `repeats` times in one process after one warm-up each:
  param    plant_rollout_param_grad_batch: J against the trajectory and dJ/dtheta [B, 2]
  control  plant_rollout_grad_batch(figure="sum"): the parent's nearest kernel, J against one state and dJ/du [B, N, 2]
Printed per run: the wall time of the call (staging included); at the end both medians and their ratio.
Then plant_calibrate_batch from the nominal drift on both data sets: wall time, evaluations, status counts and the error of the
recovered parameters against the truth."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q                       # noqa: E402
from mpc4quantum_amd import _lib, configs           # noqa: E402


def build_case(B, N):
    rng = np.random.default_rng(17)
    p = configs.build(3, batch=1)
    op0, ops = np.array(p["plant_op0"][0], complex), np.array(p["plant_ops"][0], complex)
    lv = np.arange(3.0)
    dirs = np.stack([np.diag(lv), np.diag(0.5 * lv * (lv - 1))]).astype(complex)
    scale = np.array([0.5 * p["sat"], abs(op0[2, 2].real)])
    theta = rng.uniform(-0.2, 0.2, (B, 2)) * scale
    x0 = np.empty((B, 9), complex)
    for b0 in range(0, B, 4096):                             # random density matrices
        k = min(4096, B - b0)
        M = rng.standard_normal((k, 3, 3)) + 1j * rng.standard_normal((k, 3, 3))
        rho = M @ np.conj(np.swapaxes(M, 1, 2))
        x0[b0:b0 + k] = (rho / np.trace(rho, axis1=1, axis2=2).real[:, None, None]).reshape(k, 9)
    return dict(B=B, N=N, dt=p["dt"], x0=x0, op0=op0, ops=ops, dirs=dirs, scale=scale, theta=theta,
                u=rng.uniform(-0.6 * p["sat"], 0.6 * p["sat"], (N, 2)), W=np.eye(9, dtype=complex))


def param(c, data):
    return m4q.plant_rollout_param_grad_batch(c["x0"], c["u"], c["op0"], c["ops"], c["dirs"], c["dt"], c["W"], data)


def control(c, data):
    return m4q.plant_rollout_grad_batch(c["x0"], c["u"], c["op0"], c["ops"], c["dt"], c["W"], data[:, -1], _lib.PLANT_HAMILTONIAN, figure="sum")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--sigma", type=float, default=1e-3)
    a = ap.parse_args()
    c = build_case(a.members, a.steps)
    B, N = c["B"], c["N"]
    clean = m4q.plant_rollout_batch(c["x0"], c["u"], m4q.plant_param_op0(c["op0"], c["dirs"], c["theta"]), c["ops"], c["dt"], keep="all")["xs"]
    noise = m4q.MeasurementNoise(a.sigma, seed=5, kind="hermitian")
    noisy = clean.copy()
    for t in range(1, N + 1):
        noisy[:, t] += noise.sample(np.arange(B), t, 9)
    param(c, clean), control(c, clean)                       # warm-up
    variants = (("param", param), ("control", control))
    times = {v: [] for v, _ in variants}
    for r in range(a.repeats):
        for v, fn in variants:
            t0 = time.perf_counter()
            fn(c, clean)
            times[v].append(time.perf_counter() - t0)
            print("plant_calibrate_bench repeat %d %-8s wall %9.2f ms" % (r, v, 1e3 * times[v][-1]), flush=True)
    med = {v: float(np.median(times[v])) for v in times}
    for v in times:
        t = np.array(times[v])
        print("plant_calibrate_bench B=%d N=%d %-8s wall min %.2f median %.2f max %.2f ms" % (B, N, v, 1e3 * t.min(), 1e3 * med[v], 1e3 * t.max()),
              flush=True)
    if a.repeats:
        print("plant_calibrate_bench param / control = %.2f" % (med["param"] / med["control"]), flush=True)
    for what, data in (("noise-free", clean), ("sigma %.1e" % a.sigma, noisy)):
        t0 = time.perf_counter()
        out = m4q.plant_calibrate_batch(c["x0"], c["u"], c["op0"], c["ops"], c["dirs"], c["dt"], c["W"], data,
                                        bounds=(-0.25 * c["scale"], 0.25 * c["scale"]), iters=a.iters, steps=8, tol=0.0, gtol=1e-7, step0=0.25)
        wall = time.perf_counter() - t0
        err = np.abs(out["theta"] - c["theta"]) / c["scale"]
        print("plant_calibrate_bench fit %-14s wall %8.1f ms, %d evaluations, n_iter max %d, status counts %s"
              % (what, 1e3 * wall, out["evaluations"], out["n_iter"].max(), np.bincount(out["status"], minlength=4).tolist()), flush=True)
        print("plant_calibrate_bench fit %-14s |theta - truth| / scale: median %.2e, max %.2e; cost median %.2e -> %.2e"
              % (what, np.median(err), err.max(), np.median(out["cost_hist"][:, 0]), np.median(out["cost"])), flush=True)


if __name__ == "__main__":
    main()

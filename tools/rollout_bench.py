#!/usr/bin/env python3
"""One-launch open-loop rollouts against what there was before them: N calls of m4q_plant_step_batch.

    python tools/rollout_bench.py [--repeats 3] [--case transmon|process|all] [--once]

Two cases, one seeded control sequence shared by the ensemble, uniform in +-sat:
  transmon  config 3's plant, 65,536 members, N = 80: per-member op0 = scales[:, 0] op0, u_scale = scales[:, 1:]
  process   the (16, 1) process plant of configs.synthesis, 16,384 detuned members, N = 80
Variants, alternated `repeats` times in one process after one warm-up each: the rollout returning the final figure only, the
rollout returning the whole trajectory, and the N single steps on the same data.  Printed per run: wall time of the call(s), plant
steps per second, and the bytes each variant moves over PCIe (host buffers in and out, as the one-shot entry points copy them).
--once runs every variant exactly once and times nothing: the run to put under `rocprofv3 --kernel-trace --stats`, whose kernel
statistics give plant_rollout_kernel's time against the sum over N plant_kernel launches."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q                       # noqa: E402
from mpc4quantum_amd import _lib, configs           # noqa: E402


def build_case(name, N):
    rng = np.random.default_rng(11)
    if name == "transmon":
        p = configs.build(3, batch=65536, host_models=False)
        op0 = p["scales"][:, 0, None, None] * p["plant_op0"]
        u_scale = np.ascontiguousarray(p["scales"][:, 1:])
        kind = _lib.PLANT_HAMILTONIAN
        target = np.zeros(9, complex)
        target[4] = 1                                        # |1><1|: q = the distance the closed loop's cost weighs
    else:
        p = configs.synthesis(16384, detuning_spread=0.3)
        op0 = p["plant_op0"]
        u_scale = 1 + 0.02 * rng.standard_normal((16384, 1))
        kind = _lib.PLANT_PROCESS
        target = p["target"]
    u = rng.uniform(-p["sat"], p["sat"], (N, p["dim_u"]))
    return dict(name=name, B=op0.shape[0], n=p["dim_x"], m=p["dim_u"], N=N, dt=p["dt"], kind=kind, x0=np.ascontiguousarray(p["x0"]),
                op0=np.ascontiguousarray(op0), ops=p["plant_ops"][0], u=u, u_scale=u_scale, W=np.asarray(p["Q"], complex), target=target)


def pcie_bytes(c, variant):
    B, n, m, N = c["B"], c["n"], c["m"], c["N"]
    k2 = c["op0"].shape[-1] ** 2
    plant = 16 * B * k2 * (1 + m)                            # per-member op0; the shared control operators go up once per member
    if variant == "steps":
        return N * (16 * B * n + 8 * B * m + plant), N * 16 * B * n
    up = 16 * B * n + 8 * N * m + 8 * B * m + plant + 8 * N
    if variant == "figure":
        return up + 16 * n * n + 16 * n, 8 * B
    return up, 16 * B * (N + 1) * n


def run(c, variant):
    if variant == "figure":
        return m4q.plant_rollout_batch(c["x0"], c["u"], c["op0"], c["ops"], c["dt"], c["kind"], u_scale=c["u_scale"], W=c["W"],
                                       target=c["target"], keep="none", figure="last")["q"]
    if variant == "trajectory":
        return m4q.plant_rollout_batch(c["x0"], c["u"], c["op0"], c["ops"], c["dt"], c["kind"], u_scale=c["u_scale"])["xs"][:, -1]
    x = c["x0"]
    for t in range(c["N"]):
        x = m4q.plant_step_batch(x, c["u_scale"] * c["u"][t][None], c["op0"], c["ops"], c["dt"], c["kind"])
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--case", default="all", choices=("transmon", "process", "all"))
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    variants = ("figure", "trajectory", "steps")
    for name in (("transmon", "process") if a.case == "all" else (a.case,)):
        c = build_case(name, a.steps)
        last = {v: run(c, v) for v in variants}                # warm-up (and, with --once, the only run)
        d = c["target"][None] - last["trajectory"]
        q_np = np.einsum('bj,jk,bk->b', d.conj(), c["W"], d).real
        print("rollout_bench %s B=%d n=%d m=%d N=%d: final states of rollout and %d single steps differ by %.2e (bit identical: %s), "
              "figure against NumPy %.2e" % (name, c["B"], c["n"], c["m"], c["N"], c["N"], np.abs(last["trajectory"] - last["steps"]).max(),
                                             np.array_equal(last["trajectory"], last["steps"]), np.abs(last["figure"] - q_np).max()),
              flush=True)
        for v in variants:
            up, down = pcie_bytes(c, v)
            print("rollout_bench %s %-10s PCIe bytes: %.4g MB in, %.4g MB out" % (name, v, up / 1e6, down / 1e6), flush=True)
        if a.once:
            continue
        times = {v: [] for v in variants}
        for r in range(a.repeats):
            for v in variants:
                t0 = time.perf_counter()
                run(c, v)
                times[v].append(time.perf_counter() - t0)
                print("rollout_bench %s repeat %d %-10s wall %9.2f ms  %.3e plant steps/s" %
                      (name, r, v, 1e3 * times[v][-1], c["B"] * c["N"] / times[v][-1]), flush=True)
        for v in variants:
            t = np.array(times[v])
            print("rollout_bench %s %-10s wall min %.2f median %.2f max %.2f ms (spread %.1f %%)" %
                  (name, v, 1e3 * t.min(), 1e3 * np.median(t), 1e3 * t.max(), 100 * (t.max() - t.min()) / np.median(t)), flush=True)


if __name__ == "__main__":
    main()

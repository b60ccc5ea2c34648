#!/usr/bin/env python3
"""Observed plant on the session API: the reference's crosstalk scenario on the reduced (8, 2, 1) model (two qubits, the model
sees the partial traces, the plant a sigma_z sigma_z coupling it does not know) for `--batch` members whose coupling strengths are
drawn as config 4 draws them, J_i = 1 + 0.1 xi_i (ct_i = `--ct` J_i).  Two loops over the same sessions, at the same commit:
  device   run_observed(0, n_steps) and one sync: per step the MPC launch and the plant-and-observe launch, nothing on the host;
  host     per step run(k, k + 1), sync, download of codes and controls, plant_step_batch, the NumPy lift, put_state - what mpc()
           did for this experiment class before, for the whole ensemble at once.
Wall time of each (median of `--reps` after one warm-up), their ratio, and the largest difference between the two runs.
One JSON line.
    python3 tools/observed_bench.py [--batch 65536] [--steps 6] [--horizon 8] [--reps 3] [--ct 0.1]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q  # noqa: E402
from mpc4quantum_amd import _lib, observe as ob  # noqa: E402
from mpc4quantum_amd.configs import I2, SX, SY, SZ, rx  # noqa: E402
from mpc4quantum_amd.mpc import open_session  # noqa: E402
from mpc4quantum_amd.session import EnsembleSession  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--horizon", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--ct", type=float, default=0.1)
a = ap.parse_args()

B, ns, T, dt = a.batch, a.steps, a.horizon, 0.5
J = 1 + 0.1 * np.random.default_rng(4).standard_normal(B)
L1 = [m4q.liouvillian(0 * SX), m4q.liouvillian(SX)]
L2 = [m4q.liouvillian(0 * SY), m4q.liouvillian(SY)]
zz = np.zeros((4, 4))
model = m4q.discretize_homogeneous([np.block([[L1[0], zz], [zz, L2[0]]]), np.block([[L1[1], zz], [zz, zz]]),
                                    np.block([[zz, zz], [zz, L2[1]]])], dt, 1)
sat = 2 * np.pi * 0.1
r1, r2 = rx(1e-2), rx(-1e-2)
p0, p1 = np.diag([1.0, 0]).astype(complex), np.diag([0, 1.0]).astype(complex)
z0 = np.tile(np.kron(r1 @ p0 @ r1.conj().T, r2 @ p0 @ r2.conj().T).reshape(1, 16), (B, 1))
op0 = (0.5 * a.ct * J)[:, None, None] * np.kron(SZ, SZ)[None]
ops = np.stack([0.5 * np.kron(SX, I2), 0.5 * np.kron(I2, SY)])
target = np.hstack([p1.flatten(), p1.flatten()])
X_bm, U_bm = np.tile(target[:, None], (1, ns + T + 1)), np.zeros((2, ns + T))
Q, R = np.diag([1.0, 0, 0, 1, 1, 0, 0, 1]), 1e-2 / sat ** 2 * np.eye(2)
clock = m4q.StepClock(dt, T, ns)


def device_loop(sess):
    sess.run_observed(0, ns)
    sess.sync()


def host_loop(sess):
    z = z0
    for k in range(ns):
        sess.run(k, k + 1)
        sess.sync()
        alive = sess.download(_lib.F_CODES, (B,)) == 0
        u = sess.download(_lib.F_US, (B, ns, 2))[:, k]
        z = np.where(alive[:, None], m4q.plant_step_batch(z, u, op0, ops, dt), z)
        sess.put_state(k + 1, ob.observe_reference(ob.OBSERVE_PARTIAL_TRACE, z))


def timed(loop, sess):
    times = []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        loop(sess)
        if r:
            times.append(time.perf_counter() - t0)
    return statistics.median(times)


dev = open_session(z0, model, 2, 1, X_bm, U_bm, clock, op0, ops, Q, R, Q, sat, 0.5 * sat, observe=ob.OBSERVE_PARTIAL_TRACE)
try:
    t_dev = timed(device_loop, dev)
    res_dev = dev.results()
finally:
    dev.close()
host = EnsembleSession(B, 8, 2, 1, T, ns, dt, sat, 0.5 * sat, plant_kind=_lib.PLANT_NONE, target_cols=ns + T + 1)
try:
    host.load_problem(model[None], ob.observe_batch(ob.OBSERVE_PARTIAL_TRACE, z0), X_bm, U_bm, Q, R, Q)
    t_host = timed(host_loop, host)
    res_host = host.results()
finally:
    host.close()
ok = int(np.sum((res_dev["exit_codes"] == 0) & (res_dev["steps_done"] == ns)))
print(json.dumps({"workload": "observed-crosstalk", "batch": B, "n_steps": ns, "horizon": T, "members_ok": ok,
                  "device_loop_s": round(t_dev, 5), "host_loop_s": round(t_host, 5), "host_over_device": round(t_host / t_dev, 2),
                  "max_abs_diff_us": float(np.abs(res_dev["us"] - res_host["us"]).max()),
                  "max_abs_diff_xs": float(np.abs(res_dev["xs"] - res_host["xs"]).max())}))

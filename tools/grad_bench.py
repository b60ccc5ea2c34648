#!/usr/bin/env python3
"""The control gradient of an ensemble's open-loop rollout against the rollout itself.

    python tools/grad_bench.py [--repeats 3] [--members 65536] [--steps 40] [--descent 10]

Config 3's plant (the DRAG transmon, (dim_x, dim_u) = (9, 2)), 65,536 members, N = 40: per-member op0 = scales[:, 0] op0,
u_scale = scales[:, 1:], one seeded control sequence shared by the ensemble, uniform in +-sat.  Two variants, alternated `repeats`
times in one process after one warm-up each:
  gradient  plant_rollout_grad_batch(figure="last", reduce=True): the ensemble-mean figure and its gradient [N, m]
  figure    plant_rollout_batch(keep="none", figure="last"): the landscape alone
Printed per run: the wall time of the call; at the end both medians and their ratio.
Then `--descent` projected-gradient steps on |u| <= sat with backtracking, from the configuration's zero pulse: the ensemble-mean
figure after every step."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q                       # noqa: E402
from mpc4quantum_amd import _lib, configs           # noqa: E402


def build_case(B, N):
    rng = np.random.default_rng(11)
    p = configs.build(3, batch=B, host_models=False)
    target = np.zeros(9, complex)
    target[4] = 1                                            # |1><1|: q = the distance the closed loop's cost weighs
    return dict(B=B, N=N, dt=p["dt"], sat=p["sat"], x0=np.ascontiguousarray(p["x0"]),
                op0=np.ascontiguousarray(p["scales"][:, 0, None, None] * p["plant_op0"]), ops=p["plant_ops"][0],
                u=rng.uniform(-p["sat"], p["sat"], (N, p["dim_u"])), u_scale=np.ascontiguousarray(p["scales"][:, 1:]),
                W=np.asarray(p["Q"], complex), target=target)


def gradient(c, u):
    return m4q.plant_rollout_grad_batch(c["x0"], u, c["op0"], c["ops"], c["dt"], c["W"], c["target"], _lib.PLANT_HAMILTONIAN,
                                        u_scale=c["u_scale"], figure="last", reduce=True)


def figure(c, u):
    return m4q.plant_rollout_batch(c["x0"], u, c["op0"], c["ops"], c["dt"], _lib.PLANT_HAMILTONIAN, u_scale=c["u_scale"], W=c["W"],
                                   target=c["target"], keep="none", figure="last")["q"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--descent", type=int, default=10)
    a = ap.parse_args()
    c = build_case(a.members, a.steps)
    g, q = gradient(c, c["u"]), figure(c, c["u"])            # warm-up
    print("grad_bench B=%d N=%d: q of the gradient call and of the rollout bit identical: %s; q_mean %.6f against mean(q) %.6f"
          % (c["B"], c["N"], np.array_equal(g["q"], q), g["q_mean"], q.mean()), flush=True)
    variants = (("gradient", gradient), ("figure", figure))
    times = {v: [] for v, _ in variants}
    for r in range(a.repeats):
        for v, fn in variants:
            t0 = time.perf_counter()
            fn(c, c["u"])
            times[v].append(time.perf_counter() - t0)
            print("grad_bench repeat %d %-9s wall %9.2f ms" % (r, v, 1e3 * times[v][-1]), flush=True)
    med = {v: float(np.median(times[v])) for v in times}
    for v in times:
        t = np.array(times[v])
        print("grad_bench %-9s wall min %.2f median %.2f max %.2f ms" % (v, 1e3 * t.min(), 1e3 * med[v], 1e3 * t.max()), flush=True)
    if a.repeats:
        print("grad_bench gradient / figure = %.2f" % (med["gradient"] / med["figure"]), flush=True)
    # projected gradient on the box |u| <= sat, step halved until the ensemble mean falls
    u = np.zeros_like(c["u"])
    cur = gradient(c, u)
    print("grad_bench descent step 0: q_mean %.6f, max|grad| %.3e" % (cur["q_mean"], np.abs(cur["grad"]).max()), flush=True)
    step = 0.25 * c["sat"] / max(np.abs(cur["grad"]).max(), 1e-300)
    for it in range(1, a.descent + 1):
        for _ in range(40):
            trial = np.clip(u - step * cur["grad"], -c["sat"], c["sat"])
            nxt = gradient(c, trial)
            if nxt["q_mean"] < cur["q_mean"]:
                break
            step *= 0.5
        else:
            print("grad_bench descent step %d: no lower point along the projected gradient" % it, flush=True)
            break
        u, cur = trial, nxt
        step *= 2.0
        print("grad_bench descent step %d: q_mean %.6f, max|grad| %.3e, max|u| / sat %.3f"
              % (it, cur["q_mean"], np.abs(cur["grad"]).max(), np.abs(u).max() / c["sat"]), flush=True)


if __name__ == "__main__":
    main()

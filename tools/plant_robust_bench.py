#!/usr/bin/env python3
"""One pulse optimised against an ensemble in one call, against the same loop composed from the earlier entry points
(DESIGN.md section 5.14).

    python tools/plant_robust_bench.py [--repeats 3] [--members 65536] [--steps 40] [--candidates 6] [--iters 10] [--mem 5]
                                       [--launches-only]

Config 3's plant (the DRAG transmon, (dim_x, dim_u) = (9, 2)), 65,536 detuned members (per-member op0 = scales[:, 0] op0), per-member
u_scale = scales[:, 1:], N = 40, from the configuration's zero pulse, 6 candidates per line search, 10 iterations, tol = 0.
Two variants, alternated `repeats` times in one process after one warm-up each:
  one call  plant_robust_batch: the ensemble staged once, every line search one launch of plant_rollout_multi_kernel
  composed  plant_robust_reference(evaluate=...) on plant_rollout_grad_batch(reduce=True) and one plant_rollout_batch per candidate,
            their figures weighted with numpy's dot (the composed loop's decisions may therefore differ in a last bit)
Printed per run: the wall time of the whole optimisation (each call ends in a device synchronise); at the end both medians and
their ratio, and both final costs.
Then the line search alone, by wall time per call, staging included: plant_rollout_multi_batch at S = candidates against that many
plant_rollout_batch calls.  --launches-only runs just that pair once after a warm-up: wrap it in `rocprofv3 --kernel-trace --stats`
(a run of its own) to read the kernel times of plant_rollout_multi_kernel and plant_rollout_kernel - the entry points stage their
arrays inside the call, so events around a call would time the copies too."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q                       # noqa: E402
from mpc4quantum_amd import _lib, configs           # noqa: E402


def build_case(B, N):
    p = configs.build(3, batch=B, host_models=False)
    target = np.zeros(9, complex)
    target[4] = 1                                            # |1><1|: q = the distance the closed loop's cost weighs
    return dict(B=B, N=N, dt=p["dt"], sat=p["sat"], x0=np.ascontiguousarray(p["x0"]),
                op0=np.ascontiguousarray(p["scales"][:, 0, None, None] * p["plant_op0"]), ops=p["plant_ops"][0],
                U0=np.zeros((N, p["dim_u"])), u_scale=np.ascontiguousarray(p["scales"][:, 1:]), W=np.asarray(p["Q"], complex),
                target=target)


def loop_kw(a, c):
    return dict(iters=a.iters, steps=a.candidates, mem=a.mem, step0=0.25 * c["sat"], tol=0.0)


def one_call(c, a):
    return m4q.plant_robust_batch(c["x0"], c["U0"], c["op0"], c["ops"], c["dt"], c["W"], c["target"], c["sat"], u_scale=c["u_scale"],
                                  **loop_kw(a, c))


def rollouts(c, us):
    return np.stack([m4q.plant_rollout_batch(c["x0"], u, c["op0"], c["ops"], c["dt"], _lib.PLANT_HAMILTONIAN, u_scale=c["u_scale"],
                                             W=c["W"], target=c["target"], keep="none", figure="last")["q"] for u in us], axis=1)


def composed(c, a):
    w = np.full(c["B"], 1.0 / c["B"])

    def grad_fn(U):
        out = m4q.plant_rollout_grad_batch(c["x0"], U, c["op0"], c["ops"], c["dt"], c["W"], c["target"], _lib.PLANT_HAMILTONIAN,
                                           u_scale=c["u_scale"], figure="last", reduce=True)
        return out["q_mean"], out["grad"]

    def roll_fn(us):
        return w @ rollouts(c, us)
    return m4q.plant_robust_reference(None, c["U0"], None, None, None, None, None, c["sat"], evaluate=(grad_fn, roll_fn), **loop_kw(a, c))


def multi(c, us):
    return m4q.plant_rollout_multi_batch(c["x0"], us, c["op0"], c["ops"], c["dt"], c["W"], c["target"], u_scale=c["u_scale"])


def report(name, times):
    t = np.array(times)
    print("plant_robust_bench %-9s wall min %.2f median %.2f max %.2f ms" % (name, 1e3 * t.min(), 1e3 * np.median(t), 1e3 * t.max()),
          flush=True)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--candidates", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--mem", type=int, default=5)
    ap.add_argument("--launches-only", action="store_true")
    a = ap.parse_args()
    c = build_case(a.members, a.steps)
    rng = np.random.default_rng(11)
    us = rng.uniform(-c["sat"], c["sat"], (a.candidates, a.steps, c["U0"].shape[1]))
    m, r = multi(c, us), rollouts(c, us)                     # warm-up
    print("plant_robust_bench B=%d N=%d S=%d: J of the multi launch and of %d rollouts bit identical: %s"
          % (c["B"], c["N"], a.candidates, a.candidates, np.array_equal(m["J"], r)), flush=True)
    if a.launches_only:
        multi(c, us)
        rollouts(c, us)
        return
    variants = (("one call", one_call), ("composed", composed))
    last = {v: fn(c, a) for v, fn in variants}               # warm-up
    times = {v: [] for v, _ in variants}
    for rep in range(a.repeats):
        for v, fn in variants:
            t0 = time.perf_counter()
            last[v] = fn(c, a)
            times[v].append(time.perf_counter() - t0)
            print("plant_robust_bench repeat %d %-9s wall %9.2f ms" % (rep, v, 1e3 * times[v][-1]), flush=True)
    for v in last:
        o = last[v]
        print("plant_robust_bench %-9s cost %.9f -> %.9f, n_iter %d, status %d, alpha %s"
              % (v, o["cost_hist"][0], o["cost"], o["n_iter"], o["status"], o["alpha_hist"]), flush=True)
    if a.repeats:
        med = {v: report(v, times[v]) for v in times}
        print("plant_robust_bench composed / one call = %.2f" % (med["composed"] / med["one call"]), flush=True)
    pair = {"multi": [], "rollouts": []}
    for rep in range(a.repeats):
        for v, fn in (("multi", multi), ("rollouts", rollouts)):
            t0 = time.perf_counter()
            fn(c, us)
            pair[v].append(time.perf_counter() - t0)
    if a.repeats:
        med = {v: report(v, pair[v]) for v in pair}
        print("plant_robust_bench %d rollouts / multi (calls, staging included) = %.2f" % (a.candidates, med["rollouts"] / med["multi"]),
              flush=True)


if __name__ == "__main__":
    main()

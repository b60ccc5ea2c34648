#!/usr/bin/env python3
"""One pulse optimised against an ensemble of MODELS in one call, against the same loop composed from the earlier entry points
(DESIGN.md section 5.16).

    python tools/model_robust_bench.py [--repeats 3] [--members 65536] [--steps 40] [--candidates 6] [--iters 10] [--mem 5]
                                       [--launches-only] [--shape NX,NU,ORDER]

Config 3's ensemble (the DRAG transmon, (dim_x, dim_u, order) = (9, 2, 1)): 65,536 members, per-member order-1 models from
discretize_homogeneous_batch of the detuned generators (scales[:, 0] on the drift), per-member u_scale = scales[:, 1:], N = 40, from
the configuration's zero pulse, 6 candidates per line search, 10 iterations, tol = 0.
Two variants, alternated `repeats` times in one process after one warm-up each:
  one call  model_robust_batch: the ensemble staged once, every line search one launch of model_rollout_multi_kernel
  composed  plant_robust_reference(evaluate=...) on model_rollout_grad_batch(reduce=True) and one model_rollout_batch per candidate,
            their figures weighted with ordered_weighted_sum (the decisions are those of the one call, bit for bit)
Printed per run: the wall time of the whole optimisation (each call ends in a device synchronise); at the end both medians with
minimum and maximum, their ratio, and both final costs.
Then the line search alone, by wall time per call, staging included: model_rollout_multi_batch at S = candidates against that many
model_rollout_batch calls.  --launches-only runs just that pair once after a warm-up: wrap it in `rocprofv3 --kernel-trace --stats`
(a run of its own) to read the kernel times of model_rollout_multi_kernel and model_rollout_kernel - the entry points stage their
arrays inside the call, so events around a call would time the copies too.  M4Q_LIB=tools/bin/lib<name>.so runs a variant library
(tools/build_variant.sh <name> 9_2_1 -DM4Q_DEV_MULTI_LDS: the kernel with the model's rows read from LDS at every step).
--shape NX,NU,ORDER (with --launches-only) runs the pair at another built shape, on seeded per-member models near the identity: the
kernels' times do not depend on where a model came from."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q                       # noqa: E402
from mpc4quantum_amd import configs                 # noqa: E402

ORDER = 1


def build_case(B, N):
    p = configs.build(3, batch=B, host_models=False)
    target = np.zeros(9, complex)
    target[4] = 1                                            # |1><1|: q = the distance the closed loop's cost weighs
    drift = np.ones_like(p["scales"])
    drift[:, 0] = p["scales"][:, 0]                          # the members' detuning in their models, their amplitude factors in u_scale
    models = m4q.discretize_homogeneous_batch(list(p["generators"]), p["dt"], ORDER, scales=drift)
    return dict(B=B, N=N, sat=p["sat"], x0=np.ascontiguousarray(p["x0"]), models=models, U0=np.zeros((N, p["dim_u"])),
                u_scale=np.ascontiguousarray(p["scales"][:, 1:]), W=np.asarray(p["Q"], complex), target=target)


def random_case(shape, B, N):
    """--shape: seeded per-member models near the identity, unit states, a diagonal W."""
    global ORDER
    n, m, ORDER = shape
    rng = np.random.default_rng(12)
    P = m4q.size_of_library(ORDER, m) - 1
    models = 0.15 * (rng.standard_normal((B, n, n * (1 + P))) + 1j * rng.standard_normal((B, n, n * (1 + P)))) / np.sqrt(n)
    models[:, :, :n] += np.eye(n)
    x0 = rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))
    x0 /= np.linalg.norm(x0, axis=1, keepdims=True)
    return dict(B=B, N=N, sat=0.6, x0=x0, models=models, U0=np.zeros((N, m)), u_scale=1 + 0.02 * rng.standard_normal((B, m)),
                W=np.eye(n, dtype=complex), target=np.zeros(n, complex))


def loop_kw(a, c):
    return dict(iters=a.iters, steps=a.candidates, mem=a.mem, step0=0.25 * c["sat"], tol=0.0)


def one_call(c, a):
    return m4q.model_robust_batch(c["x0"], c["U0"], c["models"], ORDER, c["W"], c["target"], c["sat"], u_scale=c["u_scale"], **loop_kw(a, c))


def rollouts(c, us):
    return np.stack([m4q.model_rollout_batch(c["x0"], u, c["models"], ORDER, u_scale=c["u_scale"], W=c["W"], target=c["target"], keep="none",
                                             figure="last")["q"] for u in us], axis=1)


def composed(c, a):
    def grad_fn(U):
        out = m4q.model_rollout_grad_batch(c["x0"], U, c["models"], ORDER, c["W"], c["target"], u_scale=c["u_scale"], figure="last",
                                           reduce=True)
        return out["q_mean"], out["grad"]

    def roll_fn(us):
        return m4q.ordered_weighted_sum(rollouts(c, us))
    return m4q.plant_robust_reference(None, c["U0"], None, None, None, None, None, c["sat"], evaluate=(grad_fn, roll_fn), **loop_kw(a, c))


def multi(c, us):
    return m4q.model_rollout_multi_batch(c["x0"], us, c["models"], ORDER, c["W"], c["target"], u_scale=c["u_scale"])


def report(name, times):
    t = np.array(times)
    print("model_robust_bench %-9s wall min %.2f median %.2f max %.2f ms" % (name, 1e3 * t.min(), 1e3 * np.median(t), 1e3 * t.max()),
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
    ap.add_argument("--shape", default=None, help="NX,NU,ORDER: another built shape, on seeded models (with --launches-only)")
    a = ap.parse_args()
    if a.shape and not a.launches_only:
        ap.error("--shape times the launches alone: pass --launches-only")
    c = random_case(tuple(int(v) for v in a.shape.split(",")), a.members, a.steps) if a.shape else build_case(a.members, a.steps)
    rng = np.random.default_rng(11)
    us = rng.uniform(-c["sat"], c["sat"], (a.candidates, a.steps, c["U0"].shape[1]))
    m, r = multi(c, us), rollouts(c, us)                     # warm-up
    print("model_robust_bench B=%d N=%d S=%d: J of the multi launch and of %d rollouts bit identical: %s"
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
            print("model_robust_bench repeat %d %-9s wall %9.2f ms" % (rep, v, 1e3 * times[v][-1]), flush=True)
    for v in last:
        o = last[v]
        print("model_robust_bench %-9s cost %.9f -> %.9f, n_iter %d, status %d, alpha %s"
              % (v, o["cost_hist"][0], o["cost"], o["n_iter"], o["status"], o["alpha_hist"]), flush=True)
    print("model_robust_bench the two runs are bit identical: %s"
          % all(np.array_equal(last["one call"][k], last["composed"][k]) for k in ("U", "cost_hist", "alpha_hist", "pgrad_hist")), flush=True)
    if a.repeats:
        med = {v: report(v, times[v]) for v in times}
        print("model_robust_bench composed / one call = %.2f" % (med["composed"] / med["one call"]), flush=True)
    pair = {"multi": [], "rollouts": []}
    for rep in range(a.repeats):
        for v, fn in (("multi", multi), ("rollouts", rollouts)):
            t0 = time.perf_counter()
            fn(c, us)
            pair[v].append(time.perf_counter() - t0)
    if a.repeats:
        med = {v: report(v, pair[v]) for v in pair}
        print("model_robust_bench %d rollouts / multi (calls, staging included) = %.2f" % (a.candidates, med["rollouts"] / med["multi"]),
              flush=True)


if __name__ == "__main__":
    main()

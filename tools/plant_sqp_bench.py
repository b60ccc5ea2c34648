#!/usr/bin/env python3
"""The SQP on the plant itself in one device call against the same iterations composed on the host.

    python tools/plant_sqp_bench.py [--batch 65536] [--horizon 40] [--iters 5,10] [--steps 6] [--repeats 3] [--parts wall,kernels]

Config 3's plant (d = 3, n = 9, m = 2), `batch` members with per-member op0 = scales[:, 0] op0 and u_scale = scales[:, 1:], one random
first guess at half the bound, the trajectory of member 0 under other random controls, shifted by 0.02, as the shared target, Q = I,
R = 0.1 I, sat the configuration's, tol = 1e-9.  Printed as measured; no figure is fixed in advance.

wall     the whole call as a caller sees it - staging in, the launches, the copy back (host clock around calls that end in a device
         synchronise) - of
           fused     plant_sqp_batch (m4q_plant_sqp_batch)
           host      the same iterations from the entry points the package had before: plant_rollout_batch for the first
                     trajectory, then per iteration plant_quad_program_batch (no gains) and one plant_rollout_batch per candidate,
                     the costs, the decision and the update in NumPy
         clipped and exact, for every count in --iters, after one warm-up each, alternating, `repeats` times; minimum, median and
         maximum.  The two are compared first: statuses, accepted step lengths, largest difference of the costs; then the ensemble
         means of the cost history and the split of the statuses are printed.
kernels  one fused call, clipped, at the first count of --iters, for a run under rocprofv3 --kernel-trace --stats (a run of its
         own): plant_factor_kernel, plant_qp_kernel and plant_step_kernel<PLANT, false> per iteration."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q                       # noqa: E402
from mpc4quantum_amd import _lib, configs           # noqa: E402

TAG = "plant_sqp_bench"
TOL = 1e-9


def problem(batch, T):
    p = configs.build(3, batch=batch, host_models=False)
    sc = p["scales"]
    op0, ops, u_scale = np.ascontiguousarray(sc[:, 0, None, None] * p["plant_op0"]), p["plant_ops"][0], np.ascontiguousarray(sc[:, 1:])
    n, m = p["dim_x"], p["dim_u"]
    rng = np.random.default_rng(62)
    U0 = 0.5 * p["sat"] * rng.uniform(-1, 1, (T, m))
    U_to = 0.9 * p["sat"] * rng.uniform(-1, 1, (T, m))
    xs = m4q.plant_rollout_batch(p["x0"][:1], U_to, op0[0], ops, p["dt"], u_scale=u_scale[:1])["xs"]
    X_bm = np.ascontiguousarray(xs[0] + 0.02)
    Q = np.ascontiguousarray(np.broadcast_to(np.identity(n, dtype=complex), (T + 1, n, n)))
    R = np.ascontiguousarray(np.broadcast_to(0.1 * np.identity(m, dtype=complex), (T, m, m)))
    return p, np.ascontiguousarray(p["x0"]), U0, op0, ops, u_scale, X_bm, np.zeros((T, m)), Q, R


def make_calls(prob, steps):
    p, x0, U0, op0, ops, u_scale, X_bm, U_bm, Q, R = prob
    B = x0.shape[0]
    T, m = U0.shape
    sat, dt = p["sat"], p["dt"]

    def fused(iters, exact):
        return m4q.plant_sqp_batch(x0, U0, op0, ops, dt, X_bm, U_bm, Q, R, sat, iters=iters, steps=steps, tol=TOL, u_scale=u_scale, exact=exact)

    def cost_of(X, U):                                           # (Q = I, R = 0.1 I, U_bm = 0)
        return (np.abs(X - X_bm) ** 2).sum(axis=(1, 2)) + 0.1 * (U ** 2).sum(axis=(1, 2))

    def roll(U):
        return m4q.plant_rollout_batch(x0, U, op0, ops, dt, u_scale=u_scale)["xs"]

    def host(iters, exact):
        U = np.ascontiguousarray(np.broadcast_to(np.clip(U0, -sat, sat), (B, T, m)))
        X = roll(U)
        J = cost_of(X, U)
        hist, alphas = np.repeat(J[:, None], iters + 1, axis=1), np.zeros((B, iters))
        status, n_iter = np.where(np.isfinite(J), 0, 3).astype(np.int32), np.zeros(B, dtype=np.int32)
        for i in range(iters):
            U_qp = m4q.plant_quad_program_batch(np.ascontiguousarray(X[:, :T]), U, op0, ops, dt, X_bm, U_bm, Q, R, sat, x_init=x0,
                                                u_scale=u_scale, exact=exact, gains=False)[1]
            D = U_qp - U
            best_J, best_a = np.full(B, np.inf), np.zeros(B)
            best_U, best_X = U.copy(), X.copy()
            for j in range(steps):
                a = 0.5 ** j
                Uj = np.clip(U + a * D, -sat, sat)
                Xj = roll(Uj)
                Jj = cost_of(Xj, Uj)
                take = np.isfinite(Jj) & (Jj < best_J)
                best_J[take], best_a[take], best_U[take], best_X[take] = Jj[take], a, Uj[take], Xj[take]
            run = status == 0
            ok = run & (best_J < J)
            status[run & ~ok] = 2
            dec = J - best_J
            U[ok], X[ok], alphas[ok, i], n_iter[ok] = best_U[ok], best_X[ok], best_a[ok], n_iter[ok] + 1
            hist[ok, i + 1:] = best_J[ok, None]
            status[ok & (dec <= TOL * J)] = 1
            J = np.where(ok, best_J, J)
        return {"X": X, "U": U, "cost": J, "cost_hist": hist, "alpha_hist": alphas, "n_iter": n_iter, "status": status}
    return fused, host


def split(status):
    return ", ".join("%d: %d" % (s, int((status == s).sum())) for s in range(4))


def wall(a):
    prob = problem(a.batch, a.horizon)
    fused, host = make_calls(prob, a.steps)
    B, (T, m), n = prob[1].shape[0], prob[2].shape, prob[1].shape[1]
    print("%s config 3 plant: B=%d T=%d n=%d m=%d, steps=%d, tol=%.0e" % (TAG, B, T, n, m, a.steps, TOL), flush=True)
    variants = [("%s, %s, %d iterations" % (path, "exact" if exact else "clipped", iters), call, iters, exact)
                for iters in a.iters for exact in (False, True) for path, call in (("fused", fused), ("host", host))]
    first = {}
    for name, call, iters, exact in variants:
        first[name] = call(iters, exact)                          # warm-up
    for iters in a.iters:
        for exact in (False, True):
            kind = "%s, %d iterations" % ("exact" if exact else "clipped", iters)
            one, two = first["fused, " + kind], first["host, " + kind]
            print("%s %s: fused against host: statuses differ for %d members, step lengths for %d, max|cost difference| %.2e (max cost %.3e)"
                  % (TAG, kind, int((one["status"] != two["status"]).sum()), int((one["alpha_hist"] != two["alpha_hist"]).any(axis=1).sum()),
                     np.abs(one["cost"] - two["cost"]).max(), np.abs(two["cost"]).max()), flush=True)
            print("%s %s: fused cost history, ensemble means: %s" % (TAG, kind, " ".join("%.6e" % v for v in one["cost_hist"].mean(axis=0))),
                  flush=True)
            print("%s %s: fused statuses (0 iterations used up, 1 converged, 2 no descent, 3 not finite): %s; iterations mean %.2f"
                  % (TAG, kind, split(one["status"]), one["n_iter"].mean()), flush=True)
    del first
    times = {name: [] for name, _, _, _ in variants}
    for r in range(a.repeats):
        for name, call, iters, exact in variants:
            t0 = time.perf_counter()
            call(iters, exact)
            times[name].append(time.perf_counter() - t0)
            print("%s repeat %d %-32s wall %10.2f ms" % (TAG, r, name, 1e3 * times[name][-1]), flush=True)
    med = {}
    for name, _, iters, _ in variants:
        t = np.array(times[name])
        med[name] = np.median(t)
        print("%s %-32s wall min %.2f median %.2f max %.2f ms, %.2f ms per iteration" %
              (TAG, name, 1e3 * t.min(), 1e3 * np.median(t), 1e3 * t.max(), 1e3 * np.median(t) / iters), flush=True)
    for iters in a.iters:
        for exact in (False, True):
            kind = "%s, %d iterations" % ("exact" if exact else "clipped", iters)
            print("%s %s: host / fused median wall %.2f" % (TAG, kind, med["host, " + kind] / med["fused, " + kind]), flush=True)


def kernels(a):
    fused, _ = make_calls(problem(a.batch, a.horizon), a.steps)
    out = fused(a.iters[0], False)
    print("%s kernels: one fused call done (B=%d T=%d, clipped, %d iterations, steps=%d): statuses %s"
          % (TAG, a.batch, a.horizon, a.iters[0], a.steps, split(out["status"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=40)
    ap.add_argument("--iters", default="5,10")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parts", default="wall", help="which parts to run, of wall and kernels")
    a = ap.parse_args()
    a.iters = [int(v) for v in a.iters.split(",")]
    parts = a.parts.split(",")
    if not parts or any(part not in ("wall", "kernels") for part in parts):
        sys.exit("%s: --parts takes wall and kernels, got %r" % (TAG, a.parts))
    if _lib.device_count() < 1:
        sys.exit("%s needs an MI355X: libm4q_hip.so has no CPU path" % TAG)
    if "wall" in parts:
        wall(a)
    if "kernels" in parts:
        kernels(a)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The QP on the plant's own linearisation in one device call against the two calls it replaces.

    python tools/plant_design_bench.py [--batch 65536] [--horizon 40] [--repeats 3] [--parts wall,kernels]

Config 3's plant (d = 3, n = 9, m = 2), `batch` members with per-member op0 = scales[:, 0] op0 and u_scale = scales[:, 1:], nominals
from their own open-loop rollouts under one random control sequence at half the bound, the nominal of member 0 shifted by 0.02 as the
shared target, Q = I, R = 0.1 I, sat the configuration's.  Printed as measured; no figure is fixed in advance.

wall     the whole call as a caller sees it - staging in, the launches, the copy back - of
           fused     plant_quad_program_batch (m4q_plant_quad_program_batch)
           two-call  plant_linearize_batch + quad_program_batch: A, B and Delta come back to the host and go up again
         each with all four outputs and without the gains (the C ABI returns X_opt, U_opt and cost always: there is no gains-only
         form), after one warm-up each, alternating, `repeats` times; minimum, median and maximum, and the workspace the fused call
         keeps per point against the bytes per point the two calls move through the host.
kernels  each path once, all outputs, for a run under rocprofv3 --kernel-trace --stats (a run of its own: the profiler's
         serialisation is not in the wall times above): plant_factor_kernel + plant_qp_kernel against plant_linearize_kernel +
         qp_kernel on the same QPs."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q                       # noqa: E402
from mpc4quantum_amd import _lib, configs           # noqa: E402
from mpc4quantum_amd.rollout import _ptr            # noqa: E402

TAG = "plant_design_bench"


def problem(batch, T):
    p = configs.build(3, batch=batch, host_models=False)
    sc = p["scales"]
    op0, ops, u_scale = np.ascontiguousarray(sc[:, 0, None, None] * p["plant_op0"]), p["plant_ops"][0], np.ascontiguousarray(sc[:, 1:])
    n, m = p["dim_x"], p["dim_u"]
    rng = np.random.default_rng(61)
    U = 0.5 * p["sat"] * rng.uniform(-1, 1, (T, m))
    xs = m4q.plant_rollout_batch(p["x0"], U, op0, ops, p["dt"], u_scale=u_scale)["xs"]
    X = np.ascontiguousarray(xs[:, :T])
    X_bm = np.ascontiguousarray(xs[0] + 0.02)
    Q = np.ascontiguousarray(np.broadcast_to(np.identity(n, dtype=complex), (T + 1, n, n)))
    R = np.ascontiguousarray(np.broadcast_to(0.1 * np.identity(m, dtype=complex), (T, m, m)))
    return p, X, U, op0, ops, u_scale, X_bm, np.ascontiguousarray(U), Q, R


def make_calls(prob):
    p, X, U, op0, ops, u_scale, X_bm, U_bm, Q, R = prob
    B, T, n = X.shape
    m = U.shape[1]
    sat, dt = p["sat"], p["dt"]
    x_init = np.ascontiguousarray(X[:, 0])

    def fused(gains):
        return m4q.plant_quad_program_batch(X, U, op0, ops, dt, X_bm, U_bm, Q, R, sat, u_scale=u_scale, gains=gains)

    def two_call(gains):
        A, Bm, D = m4q.plant_linearize_batch(X, U, op0, ops, dt, u_scale=u_scale)
        if gains:
            return m4q.quad_program_batch(x_init, X_bm[None], U_bm[None], Q, R, A, Bm, D, None, sat, None)
        Xo, Uo, cost = np.empty((B, T + 1, n), dtype=complex), np.empty((B, T, m)), np.empty(B)
        _lib.check(_lib.lib().m4q_quad_program_batch(B, n, m, T, 0, float(sat), 0.0, _ptr(x_init), _ptr(X_bm), _ptr(U_bm), 0, _ptr(Q), _ptr(R),
                                                     _ptr(A), _ptr(Bm), _ptr(D), None, _ptr(Xo), _ptr(Uo), _ptr(cost), None))
        return Xo, Uo, cost, None
    return fused, two_call


def wall(a):
    prob = problem(a.batch, a.horizon)
    fused, two_call = make_calls(prob)
    B, T, n = prob[1].shape
    m, d = prob[2].shape[1], 3
    print("%s config 3 plant: B=%d T=%d n=%d m=%d, %d points" % (TAG, B, T, n, m, B * T), flush=True)
    ws, host = 16 * (d * d + n * m + n), 16 * (n * n + n * m + n)
    print("%s per point: fused workspace %d B (U_t %d + B_t %d + Delta_t %d) against %d B through the host, down and up again (A_t %d)"
          % (TAG, ws, 16 * d * d, 16 * n * m, 16 * n, host, 16 * n * n), flush=True)
    variants = [("fused, all outputs", lambda: fused(True)), ("two-call, all outputs", lambda: two_call(True)),
                ("fused, no gains", lambda: fused(False)), ("two-call, no gains", lambda: two_call(False))]
    first = {}
    for name, call in variants:
        first[name] = call()                                      # warm-up
    for kind in ("all outputs", "no gains"):
        one, two = first["fused, " + kind], first["two-call, " + kind]
        same = all(g is None or np.array_equal(g, w) for g, w in zip(one, two))
        worst = max(np.abs(g - w).max() for g, w in zip(one, two) if g is not None)
        print("%s %s: fused against two-call max|difference| %.2e, bit-identical: %s" % (TAG, kind, worst, same), flush=True)
    del first
    times = {name: [] for name, _ in variants}
    for r in range(a.repeats):
        for name, call in variants:
            t0 = time.perf_counter()
            call()
            times[name].append(time.perf_counter() - t0)
            print("%s repeat %d %-22s wall %9.2f ms" % (TAG, r, name, 1e3 * times[name][-1]), flush=True)
    med = {}
    for name, _ in variants:
        t = np.array(times[name])
        med[name] = np.median(t)
        print("%s %-22s wall min %.2f median %.2f max %.2f ms, %.1f ns per point" %
              (TAG, name, 1e3 * t.min(), 1e3 * np.median(t), 1e3 * t.max(), 1e9 * np.median(t) / (B * T)), flush=True)
    for kind in ("all outputs", "no gains"):
        print("%s %s: two-call / fused median wall %.2f" % (TAG, kind, med["two-call, " + kind] / med["fused, " + kind]), flush=True)


def kernels(a):
    fused, two_call = make_calls(problem(a.batch, a.horizon))
    fused(True)
    two_call(True)
    print("%s kernels: one fused call and one two-call pass done (B=%d T=%d)" % (TAG, a.batch, a.horizon), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parts", default="wall", help="which parts to run, of wall and kernels")
    a = ap.parse_args()
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

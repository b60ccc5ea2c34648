#!/usr/bin/env python3
"""The plant's own linearisation for an ensemble in one launch: its cost, what it is for, what it shows.

    python tools/plant_linearize_bench.py [--batch 65536] [--points 40] [--repeats 3] [--members 4096] [--steps 8] [--parts gap,law,timing]

Three parts, each printed as measured; no figure is fixed in advance.
1. Config 3's plant (d = 3, m = 2), `batch` members with per-member op0 = scales[:, 0] op0 and u_scale = scales[:, 1:], linearised at
   the first `points` states of their open-loop rollouts under one random control sequence: the wall time of
   plant_linearize_batch for B and Delta only, and for all three outputs, alternated `repeats` times after one warm-up each, with
   the bytes that come back and bytes / wall time.  The wall time is the whole call - staging in, the launch, the copy back - as a
   caller sees it: the Jacobians pass through the host.
2. max|A_model - A_plant| and max|B_model - B_plant| for the order-1 and order-2 Taylor/Dyson models (discretize_homogeneous of the
   plant's own operators, so that truncation is the only difference) at configs 1-4's own dt, over 8 points of a rollout under
   random controls inside the bound.  The model's Jacobians are formed on the host from its blocks.
3. Config 3's ensemble (`members` of them, each with its own drift scale and drive calibration, from a perturbed x0) run through
   plant_feedback_batch under three laws around member 0's `steps`-step trajectory, the trajectory itself as target, Q = I,
   R = 0.1 I: open loop (zero gains), FeedbackLaw.along_trajectory on member 0's order-1 model, and
   FeedbackLaw.along_plant_trajectory on member 0's plant.  Printed: each law's affine column, the landscape of the final
   distance |x_N - X_nom[N]| over the ensemble, and the same distance for member 0 started on the nominal x0 itself."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q                       # noqa: E402
from mpc4quantum_amd import _lib, configs           # noqa: E402

TAG = "plant_linearize_bench"


def ensemble(batch):
    """Config 3's plant for `batch` members: (p, op0 [B, d, d], ops [m, d, d], u_scale [B, m])."""
    p = configs.build(3, batch=batch, host_models=False)
    sc = p["scales"]
    return p, np.ascontiguousarray(sc[:, 0, None, None] * p["plant_op0"]), p["plant_ops"][0], np.ascontiguousarray(sc[:, 1:])


def timing(a):
    p, op0, ops, u_scale = ensemble(a.batch)
    n, m, T = p["dim_x"], p["dim_u"], a.points
    rng = np.random.default_rng(31)
    U = 0.5 * p["sat"] * rng.uniform(-1, 1, (T, m))
    X = np.ascontiguousarray(m4q.plant_rollout_batch(p["x0"], U, op0, ops, p["dt"], u_scale=u_scale)["xs"][:, :T])
    variants = (("B, Delta", ("B", "Delta"), 16 * n * (m + 1)), ("A, B, Delta", ("A", "B", "Delta"), 16 * n * (n + m + 1)))
    print("%s config 3 plant: B=%d T=%d n=%d m=%d, %d points" % (TAG, a.batch, T, n, m, a.batch * T), flush=True)

    def call(outputs):
        return m4q.plant_linearize_batch(X, U, op0, ops, p["dt"], u_scale=u_scale, outputs=outputs)
    for _, outputs, _ in variants:
        call(outputs)                                           # warm-up
    times = {name: [] for name, _, _ in variants}
    for r in range(a.repeats):
        for name, outputs, _ in variants:
            t0 = time.perf_counter()
            call(outputs)
            times[name].append(time.perf_counter() - t0)
            print("%s repeat %d %-12s wall %9.2f ms" % (TAG, r, name, 1e3 * times[name][-1]), flush=True)
    for name, _, per_point in variants:
        t = np.array(times[name])
        out_bytes = per_point * a.batch * T
        print("%s %-12s output %.3f GB, wall min %.2f median %.2f max %.2f ms, output bytes / median wall %.2f GB/s, %.1f ns per point" %
              (TAG, name, out_bytes / 1e9, 1e3 * t.min(), 1e3 * np.median(t), 1e3 * t.max(), out_bytes / np.median(t) / 1e9,
               1e9 * np.median(t) / (a.batch * T)), flush=True)


def model_jacobians(model, order, x, u):
    """A(u) and df/du at (x, u) of x+ = A [x ; lift_u(u) (x) x], from the model's blocks (host)."""
    n, m = x.shape[0], u.shape[0]
    powers = m4q.create_power_list(order, m)[1:]
    A = model[:, :n].astype(complex)
    Bm = np.zeros((n, m), dtype=complex)
    for i, e in enumerate(powers):
        blk = model[:, (1 + i) * n:(2 + i) * n]
        A = A + float(np.prod(u ** e)) * blk
        for k in range(m):
            if e[k] > 0:
                de = e.copy()
                de[k] -= 1
                Bm[:, k] += e[k] * float(np.prod(u ** de)) * (blk @ x)
    return A, Bm


def gap_table():
    print("%s model against plant at the configurations' own dt (8 points of a rollout under random controls inside the bound)" % TAG)
    for config in (1, 2, 3, 4):
        p = configs.build(config, batch=1)
        n, m, dt = p["dim_x"], p["dim_u"], p["dt"]
        op0, ops = p["plant_op0"][0], p["plant_ops"][0]
        rng = np.random.default_rng(40 + config)
        U = p["sat"] * rng.uniform(-1, 1, (8, m))
        X = m4q.plant_rollout_batch(p["x0"][:1], U, op0, ops, dt)["xs"][:, :8]
        A, Bm, _ = m4q.plant_linearize_batch(X, U, op0, ops, dt)
        gens = [m4q.liouvillian(op0)] + [m4q.liouvillian(h) for h in ops]
        for order in (1, 2):
            model = m4q.discretize_homogeneous(gens, dt, order)
            gA = gB = 0.0
            for t in range(8):
                Am, Bmod = model_jacobians(model, order, X[0, t], U[t])
                gA, gB = max(gA, np.abs(Am - A[0, t]).max()), max(gB, np.abs(Bmod - Bm[0, t]).max())
            print("%s config %d (n=%d m=%d dt=%g) order %d: max|A_model - A_plant| %.3e  max|B_model - B_plant| %.3e  (max|B_plant| %.3e)"
                  % (TAG, config, n, m, dt, order, gA, gB, np.abs(Bm).max()), flush=True)


def landscape(name, dist):
    print("%s %-22s |x_N - X_nom[N]|: min %.3e  median %.3e  mean %.3e  90 %% %.3e  max %.3e" %
          (TAG, name, dist.min(), np.median(dist), dist.mean(), np.quantile(dist, 0.9), dist.max()), flush=True)


def three_way(a):
    p, op0, ops, u_scale = ensemble(a.members)
    n, m, N, sat, dt = p["dim_x"], p["dim_u"], a.steps, p["sat"], p["dt"]
    rng = np.random.default_rng(51)
    U_nom = 0.5 * sat * rng.uniform(-1, 1, (N, m))
    X_nom = m4q.plant_rollout_batch(p["x0"][:1], U_nom, op0[:1], ops, dt, u_scale=u_scale[:1])["xs"][0]
    Q, R = np.identity(n), 0.1 * np.identity(m)
    sc0 = p["scales"][0]
    model0 = m4q.discretize_homogeneous([sc0[k] * p["generators"][k] for k in range(1 + m)], dt, 1)
    laws = (("open loop", m4q.FeedbackLaw(np.zeros((N, n + 1, m)), X_nom, U_nom, sat)),
            ("order-1 model's law", m4q.FeedbackLaw.along_trajectory(model0, 1, X_nom, U_nom, X_nom, U_nom, Q, R, sat)),
            ("plant's law", m4q.FeedbackLaw.along_plant_trajectory(op0[0], ops, dt, X_nom, U_nom, X_nom, U_nom, Q, R, sat,
                                                                   u_scale=u_scale[:1])))
    d = p["d"]
    G = 0.02 * (rng.standard_normal((a.members, d, d)) + 1j * rng.standard_normal((a.members, d, d)))
    x0 = p["x0"] + (0.5 * (G + G.conj().transpose(0, 2, 1))).reshape(a.members, n)
    print("%s config 3 ensemble: B=%d members (own drift scale and drive calibration, x0 perturbed by 0.02), N=%d steps around member 0's "
          "trajectory" % (TAG, a.members, N), flush=True)
    for name, law in laws:
        out = m4q.plant_feedback_batch(x0, law, op0, ops, dt, u_scale=u_scale, W=np.identity(n, dtype=complex), target=X_nom[N],
                                       keep="none", figure="last")
        print("%s %-22s affine column %.3e, max|K| %.3g, bounds active per member: mean %.2f of %d, members lost: %d" %
              (TAG, name, np.abs(law.gains[:, n]).max(), np.abs(law.gains[:, :n]).max(), out["clipped"].mean(), N * m,
               int((out["status"] != 0).sum())), flush=True)
        landscape(name, np.sqrt(np.maximum(out["q"], 0.0)))
        own = m4q.plant_feedback_batch(p["x0"][:1], law, op0[:1], ops, dt, u_scale=u_scale[:1], W=np.identity(n, dtype=complex),
                                       target=X_nom[N], keep="none", figure="last")
        print("%s %-22s member 0 from the nominal x0 itself: |x_N - X_nom[N]| %.3e" % (TAG, name, np.sqrt(max(own["q"][0], 0.0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--points", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--parts", default="gap,law,timing", help="which parts to run, of gap (2), law (3), timing (1)")
    a = ap.parse_args()
    parts = a.parts.split(",")
    if not parts or any(part not in ("gap", "law", "timing") for part in parts):
        sys.exit("%s: --parts takes gap, law and timing, got %r" % (TAG, a.parts))
    if _lib.device_count() < 1:
        sys.exit("%s needs an MI355X: libm4q_hip.so has no CPU path" % TAG)
    if "gap" in parts:
        gap_table()
    if "law" in parts:
        three_way(a)
    if "timing" in parts:
        timing(a)


if __name__ == "__main__":
    main()

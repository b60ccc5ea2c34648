#!/usr/bin/env python3
"""A stored feedback law on an ensemble in one launch, against the open-loop rollout of the same ensemble.

    python tools/feedback_bench.py [--batch 65536] [--repeats 3] [--sigma 0.01]

Config 3's plant, `batch` members with per-member op0 = scales[:, 0] op0 and u_scale = scales[:, 1:].  Member 0's closed loop
(mpc_batch, one member) gives the nominal trajectory; FeedbackLaw.along_trajectory builds the law around it on member 0's model
(the QP's benchmark is the nominal trajectory itself, bounds and band the configuration's).  Printed: the landscape of the final
figure q_N = Re((x_N - f)^H Q (x_N - f)) over the ensemble for the nominal controls applied open loop, for the law, and for the law
under hermitian measurement noise; then, alternated `repeats` times after one warm-up each, the wall time of the feedback launch
against plant_rollout_batch on the same data (figure only: the same bytes come back).  No ratio is fixed in advance."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q                       # noqa: E402
from mpc4quantum_amd import _lib, configs           # noqa: E402


def landscape(name, q):
    print("feedback_bench %-22s q_N: min %.3e  median %.3e  mean %.3e  90 %% %.3e  max %.3e" %
          (name, q.min(), np.median(q), q.mean(), np.quantile(q, 0.9), q.max()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.01)
    a = ap.parse_args()
    p = configs.build(3, batch=a.batch, host_models=False)
    n, m, N, sat, du = p["dim_x"], p["dim_u"], p["n_steps"], p["sat"], p["du"]
    sc = p["scales"]
    op0 = np.ascontiguousarray(sc[:, 0, None, None] * p["plant_op0"])
    u_scale = np.ascontiguousarray(sc[:, 1:])
    model0 = m4q.discretize_homogeneous([sc[0, k] * p["generators"][k] for k in range(1 + m)], p["dt"], 1)
    clock = m4q.StepClock(p["dt"], p["horizon"], N)
    run0 = m4q.mpc_batch(p["x0"][:1], model0[None], m, 1, p["X_targ"], p["U_targ"], clock, op0[:1], p["plant_ops"], p["Q"], p["R"],
                         p["Qf"], sat, du)
    assert run0["steps_done"][0] == N and run0["exit_codes"][0] == 0, (run0["steps_done"], run0["exit_codes"])
    X_nom, U_nom = np.ascontiguousarray(run0["xs"][0].T), np.ascontiguousarray(run0["us"][0].T)
    law = m4q.FeedbackLaw.along_trajectory(model0, 1, X_nom, U_nom, X_nom, U_nom, p["Q"], p["R"], sat, du=du, u_prev=np.zeros(m))
    W = np.asarray(p["Q"], complex)
    target = np.ascontiguousarray(p["X_targ"][:, 0])
    noise = m4q.MeasurementNoise(a.sigma, 2024, "hermitian")
    kw = dict(u_scale=u_scale, W=W, target=target, keep="none", figure="last")

    def open_loop():
        return m4q.plant_rollout_batch(p["x0"], U_nom, op0, p["plant_ops"][0], p["dt"], _lib.PLANT_HAMILTONIAN, **kw)

    def closed(nz=None, controls=False):
        return m4q.plant_feedback_batch(p["x0"], law, op0, p["plant_ops"][0], p["dt"], _lib.PLANT_HAMILTONIAN, noise=nz, controls=controls,
                                        **kw)
    print("feedback_bench config 3 plant: B=%d n=%d m=%d N=%d, law along member 0's MPC run (q_N of that run: %.3e), |K| max %.3g" %
          (a.batch, n, m, N, np.real((X_nom[N] - target).conj() @ W @ (X_nom[N] - target)), np.abs(law.gains).max()), flush=True)
    ol, fb, fn = open_loop(), closed(), closed(noise)           # (the warm-up of every variant as well)
    landscape("open loop", ol["q"])
    landscape("feedback", fb["q"])
    landscape("feedback, sigma %g" % a.sigma, fn["q"])
    for name, out in (("feedback", fb), ("feedback, sigma %g" % a.sigma, fn)):
        print("feedback_bench %-22s bounds active per member: mean %.2f of %d, members lost: %d" %
              (name, out["clipped"].mean(), N * m, int((out["status"] != 0).sum())), flush=True)
    times = {"rollout": [], "feedback": [], "feedback+noise": []}
    for r in range(a.repeats):
        for name, fn_ in (("rollout", open_loop), ("feedback", closed), ("feedback+noise", lambda: closed(noise))):
            t0 = time.perf_counter()
            fn_()
            times[name].append(time.perf_counter() - t0)
            print("feedback_bench repeat %d %-15s wall %9.2f ms" % (r, name, 1e3 * times[name][-1]), flush=True)
    for name, t in times.items():
        t = np.array(t)
        print("feedback_bench %-15s wall min %.2f median %.2f max %.2f ms" % (name, 1e3 * t.min(), 1e3 * np.median(t), 1e3 * t.max()),
              flush=True)
    print("feedback_bench feedback / rollout (medians): %.3f, with noise %.3f" %
          (np.median(times["feedback"]) / np.median(times["rollout"]), np.median(times["feedback+noise"]) / np.median(times["rollout"])),
          flush=True)


if __name__ == "__main__":
    main()

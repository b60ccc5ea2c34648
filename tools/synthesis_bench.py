#!/usr/bin/env python3
"""Gate-synthesis ensemble on the session API (M4Q_PLANT_PROCESS, shapes (16, 1, k)): configs.synthesis - the reference's NOT-gate
scenario (n = 16, one drive, T = 15, 50 MPC steps) with per-member detunings of the plant - for `--batch` members at each
`--orders`; kernel time per run from m4q_session_kernel_ms (HIP events around the launches), best of `--reps` after one warm-up,
and the oracle's (NumPy) host rate on `--oracle-members` members of the same run for comparison.  One JSON line per order.
    python3 tools/synthesis_bench.py [--batch 65536] [--orders 1,2] [--reps 3] [--oracle-members 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q  # noqa: E402
from mpc4quantum_amd import _lib, configs  # noqa: E402
from mpc4quantum_amd.mpc import open_session  # noqa: E402
from oracle import m4q_oracle as orc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--orders", default="1,2")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--spread", type=float, default=0.3, help="detuning spread of the plant (rad / time unit)")
ap.add_argument("--oracle-members", type=int, default=2)
a = ap.parse_args()

for order in [int(o) for o in a.orders.split(",")]:
    p = configs.synthesis(a.batch, order, detuning_spread=a.spread)
    B, ns, T = p["batch"], p["n_steps"], p["horizon"]
    clock = m4q.StepClock(p["dt"], T, ns)
    sess = open_session(p["x0"], p["models"], 1, order, p["X_targ"], p["U_targ"], clock, p["plant_op0"], p["plant_ops"], p["Q"],
                        p["R"], p["Qf"], p["sat"], p["du"], plant_kind=_lib.PLANT_PROCESS)
    try:
        info = sess.info()
        times = []
        for r in range(a.reps + 1):
            sess.kernel_ms()
            sess.run(0, ns)
            sess.sync()
            ms, launches = sess.kernel_ms()
            if r:
                times.append(ms)
        res = sess.results()
        path = sess.path_detail()
    finally:
        sess.close()
    ok = int(np.sum((res["exit_codes"] == 0) & (res["steps_done"] == ns)))
    best = min(times)
    # the oracle on the first members of the same ensemble: host seconds per member, same loop (qp_mode "qp")
    eye = np.identity(2)
    model = orc.OracleDMDc(16, 16, p["models"].shape[2] - 16, p["models"][0])
    t0 = time.perf_counter()
    for b in range(a.oracle_members):
        Ls = [np.kron(-1j * (np.kron(h, eye) - np.kron(eye, h.conj())), np.identity(4)) for h in (p["plant_op0"][b], p["plant_ops"][0, 0])]
        orc.mpc(p["x0"][b], 1, order, p["X_targ"], p["U_targ"], orc.OracleClock(p["dt"], T, ns), orc.OracleLExperiment(Ls[0], Ls[1:]),
                model, p["Q"], p["R"], p["Qf"], sat=p["sat"], du=p["du"])
    s_per_member = (time.perf_counter() - t0) / max(1, a.oracle_members)
    print(json.dumps({"workload": "synthesis", "order": order, "batch": B, "n_steps": ns, "horizon": T, "path": path,
                      "kernel_ms": round(best, 3), "kernel_ms_reps": [round(t, 3) for t in times], "launches": launches,
                      "horizon_steps_per_s": B * ns * T / (best * 1e-3), "members_ok": ok, "grid": info["grid"],
                      "lds_bytes": info["lds_bytes"], "oracle_s_per_member": round(s_per_member, 3),
                      "oracle_horizon_steps_per_s": ns * T / s_per_member}), flush=True)

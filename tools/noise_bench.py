#!/usr/bin/env python3
"""What the measurement noise costs: config 3, 65,536 members, sigma = 1e-2.

    python tools/noise_bench.py [--batch 65536] [--repeats 3] [--sigma 1e-2]

Launch time (HIP events, m4q_session_kernel_ms) of the whole 20-step run, variants alternated `repeats` times in one process:
noise off against "hermitian" on the path the configuration gets by default (the headline path), and the complex path's own
noise-off time against "iid".  Noise perturbs the warm starts, so the QP solves of each run (sum of qp_solves over members and
steps) and m4q_session_qp_stats stand beside each time.  Last: m4q_noise_sample_batch for batch x 9 (wall time of the call: the
kernel, one 8-byte sigma in and 16 batch n bytes out)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc4quantum_amd as m4q                       # noqa: E402
from mpc4quantum_amd import _lib, configs           # noqa: E402
from mpc4quantum_amd.mpc import open_session        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=1e-2)
    a = ap.parse_args()
    p = configs.build(3, batch=a.batch, host_models=False)
    clock = m4q.StepClock(p["dt"], p["horizon"], p["n_steps"])

    def session(noise, **kw):
        return open_session(p["x0"], None, p["dim_u"], p["order"], p["X_targ"], p["U_targ"], clock, p["plant_op0"], p["plant_ops"],
                            p["Q"], p["R"], p["Qf"], p["sat"], p["du"], generators=p["generators"], scales=p["scales"], noise=noise,
                            **kw)
    variants = [("off", None, {}), ("hermitian", m4q.MeasurementNoise(a.sigma, 1, "hermitian"), {}),
                ("complex-off", None, dict(force_complex=True)), ("iid", m4q.MeasurementNoise(a.sigma, 1, "iid"), {})]
    sessions = [(name, session(noise, **kw)) for name, noise, kw in variants]
    try:
        for name, s in sessions:                    # warm-up: clocks, code objects, first-touch of the workspace
            s.run(0, p["n_steps"])
            s.sync()
            s.kernel_ms()
        for r in range(a.repeats):
            for name, s in sessions:
                s.run(0, p["n_steps"])
                s.sync()
                ms, launches = s.kernel_ms()
                solves = int(s.download(_lib.F_QP_SOLVES, (a.batch, p["n_steps"])).sum(dtype=np.int64))
                codes = s.download(_lib.F_CODES, (a.batch,))
                print("noise_bench repeat %d %-12s path %-15s launch %8.3f ms (%d launch)  qp_solves %d  qp_stats %s  nonzero codes %d"
                      % (r, name, s.path_detail(), ms, launches, solves, s.qp_stats(), int(np.count_nonzero(codes))), flush=True)
    finally:
        for _, s in sessions:
            s.close()
    n = p["dim_x"]
    L = _lib.lib()
    out = np.empty((a.batch, n), dtype=np.complex128)
    sg = np.full(1, a.sigma)
    for kind, mode in (("iid", _lib.NOISE_IID), ("hermitian", _lib.NOISE_HERMITIAN)):
        for r in range(a.repeats + 1):              # (the first call loads the code object)
            t0 = time.perf_counter()
            _lib.check(L.m4q_noise_sample_batch(a.batch, n, mode, sg.ctypes.data_as(_lib._dp), 0, 1, 0, 1, out.ctypes.data_as(_lib._dp)))
            dt = time.perf_counter() - t0
            if r:
                print("noise_bench m4q_noise_sample_batch %-9s %d x %d: %.3f ms per call" % (kind, a.batch, n, 1e3 * dt), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measurement noise in the on-device closed loops (slsqp_cl_set_meas_noise): what the option costs, and what the loop does
when the controller is not given the plant's state.  The rocket closed loop of bench.py (N = 20, the script's x0) as ONE persistent launch.

    python scripts/bench_meas_noise.py [--batch 4096] [--steps 30] [--N 20] [--reps 7]
    python scripts/bench_meas_noise.py --study [--seeds 1024] [--amp 0 0.5 1 2]

Timing (default): three handles -- the option never set, an all-zero table, amp = 1 (x_meas = x_plant + E[0] v, v uniform in [-1,1]) -- run in turn
--reps times after one uncounted round that warms the code objects, so drift of the machine reaches all three alike.  One JSON line per handle:
  ms_per_step        median over the runs of the wall time from reset's return to the end of slsqp_cl_run (the upload of the samples included; the
                     call ends in a stream synchronise), per closed-loop step; ms_per_step_runs holds every run
  spread             max - min of the runs
and a last line with the differences of the medians against the option-off handle, next to the spread of the option-off runs.
The nominal trajectory of the first step is solved once, without the option, and handed to every run.

--study: run_monte_carlo over --seeds seeds at every --amp, with the strict stage-0 gate and with X0_BOX_TOL_OSQP_DEFAULT.  One JSON line each:
  solved_share       fraction of the MPC steps whose solve succeeded
  margin_min         smallest constraint_margin of the TRUE state and the applied input against the model's box (negative: outside)
  x0_refused_share   share of the steps whose first QP was refused at x0 (its stage-0 violation above the gate)
  x0_violation_max   largest stage-0 violation of the measurement the first QPs recorded
amp = 0 runs with the option on and a table of zeros."""
import argparse
import json
import os
import sys
import time

import numpy as np


def timing(a):
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, disturbance_stream, get_model, meas_noise_table, measurement_stream
    m = get_model("rocket")
    B, N, steps = a.batch, a.N, a.steps
    x0 = np.tile(np.asarray(m.extra["x0"], dtype=float), (B, 1))
    W = np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)
    V = np.stack([measurement_stream(s, steps + 1, m.nw) for s in range(B)])
    cl = ClosedLoopMPC(m, N, B)
    cl.reset(x0, solve_nominal=True, continuation=2)
    X_nom, U_nom = cl.f.get("nominal_x", (N + 1, m.nx)), cl.f.get("nominal_u", (N, m.nu))
    cl.close()
    settings = [("off", None), ("zero_table", np.zeros((1, m.nx))), ("amp_1", meas_noise_table(m, V, 1.0))]
    handles = []
    for label, table in settings:
        cl = ClosedLoopMPC(m, N, B) if table is None else ClosedLoopMPC(m, N, B, meas_noise=table)      # (off: the option is not named at all)
        mark = {}

        def timed_reset(*args, _r=cl.reset, _m=mark, **kw):
            r = _r(*args, **kw)
            _m["t0"] = time.perf_counter()
            return r

        def timed_log_result(*args, _l=cl._log_result, _m=mark, **kw):
            _m["t1"] = time.perf_counter()
            return _l(*args, **kw)
        cl.reset, cl._log_result = timed_reset, timed_log_result
        handles.append((label, cl, mark, [], {}))
    for rep in range(a.reps + 1):
        for label, cl, mark, runs, last in handles:
            out = cl.run_decoupled(x0, steps, W, X_nom, U_nom)
            if rep:
                runs.append(1e3 * (mark["t1"] - mark["t0"]) / steps)
            last["out"] = out
    med = {}
    for label, cl, mark, runs, last in handles:
        cl.close()
        out = last["out"]
        med[label] = float(np.median(runs))
        print(json.dumps(dict(setting=label, batch=B, N=N, steps=steps, ms_per_step=med[label], spread=float(max(runs) - min(runs)), ms_per_step_runs=[round(r, 4) for r in runs],
                              solved_share=float(out["success"].mean()), launch_ms=out["loop_stats"]["launch_ms"])), flush=True)
    off_runs = handles[0][3]
    print(json.dumps(dict(summary="median ms_per_step against the option-off handle", zero_table_minus_off=med["zero_table"] - med["off"], amp_1_minus_off=med["amp_1"] - med["off"],
                          off_spread=float(max(off_runs) - min(off_runs)), off_std=float(np.std(off_runs)))), flush=True)


def study(a):
    from robust_nonlinear_mpc_amd import X0_BOX_TOL_OSQP_DEFAULT, constraint_margin, get_model, run_monte_carlo
    m = get_model("rocket")
    x0 = np.asarray(m.extra["x0"], dtype=float)
    g = np.asarray(m.g, dtype=float)[None, :]
    for tol_name, tol in (("strict", 0.0), ("osqp_default", X0_BOX_TOL_OSQP_DEFAULT)):
        for amp in a.amp:
            r = run_monte_carlo(m, a.N, np.arange(a.seeds), a.steps, x0, solve_nominal=True, continuation=2, x0_box_tol=tol, meas_noise=float(amp))
            margin = constraint_margin(m, g, r["state_trajectory"], r["input_trajectory"])
            v0 = r["x0_violation"][:, :, 0]
            print(json.dumps(dict(x0_box_tol=tol_name, amp=float(amp), seeds=a.seeds, N=a.N, steps=a.steps, solved_share=float(r["success"].mean()),
                                  margin_min=float(np.nanmin(margin)), x0_refused_share=float(np.mean(v0 > max(1e-9, tol))), x0_violation_max=float(v0.max()),
                                  meas_error_max=float(np.abs(r["measured_trajectory"] - r["state_trajectory"]).max()),
                                  nlp_ok=float(np.mean(r["nlp_status"] == 0)))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--study", action="store_true")
    ap.add_argument("--seeds", type=int, default=1024)
    ap.add_argument("--amp", type=float, nargs="+", default=[0.0, 0.5, 1.0, 2.0])
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    (study if a.study else timing)(a)


if __name__ == "__main__":
    main()

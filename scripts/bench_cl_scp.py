#!/usr/bin/env python3
"""Closed loops with several SCP iterations / fast-SLS steps per MPC step: the persistent launch (slsqp_cl_run_scp) against the two step-by-step
paths, in one process on identical inputs:
  (a) run_on_device, one slice            one slsqp_cl_step per MPC step for the whole batch
  (b) run_monte_carlo(budget_ms=0, slices=3)   the same on three free-running slices
  (c) run_decoupled                       ONE persistent launch (k_cl_loop_scp)
Each is warmed on a disjoint seed batch, then the wall time of the whole run (handle, nominal initialiser, loop, read-back) is taken `--repeats`
times; (c)'s outputs must equal (a)'s bit for bit.  One JSON line: median and min-max per path, ms per MPC step, wave_busy_frac of (c).

    python scripts/bench_cl_scp.py --model pendulum  --batch 1024 --steps 60            # script settings (rti 3, 2 fast-SLS steps)
    python scripts/bench_cl_scp.py --model quadrotor --batch 2048 --steps 30
    python scripts/bench_cl_scp.py --model rocket    --batch 4096 --steps 10 --rti -1 --rti-steps 1      # SCP converge mode (BASELINE config 4)
    python scripts/bench_cl_scp.py --model rocket    --batch 4096 --steps 10 --rti 1 --sls-converge      # fast-SLS converge mode (fast_SLS.solve's default)
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robust_nonlinear_mpc_amd import get_model, run_monte_carlo  # noqa: E402
from robust_nonlinear_mpc_amd.monte_carlo import _run_slice  # noqa: E402

KEYS = ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x", "backoff_trajectory_u", "success",
        "scp_iterations", "primal_infeasibility")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="pendulum", choices=["pendulum", "quadrotor", "rocket"])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--N", type=int, default=None)
    ap.add_argument("--rti", type=int, default=None, help="SCP iterations per MPC step (<= 0: converge mode); default: the script's")
    ap.add_argument("--rti-steps", type=int, default=None, help="fast-SLS steps per solve; default: the script's")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warm-batch", type=int, default=64)
    ap.add_argument("--paths", default="abc")
    ap.add_argument("--sls-converge", action="store_true",
                    help="fast-SLS converge mode (fast_sls_rti_steps None: every solve iterates to convergence, --rti-steps is ignored); (c) then is the "
                    "persistent launch with every instance iterating on its own (run_decoupled's persistent_converge)")
    a = ap.parse_args()
    m = get_model(a.model)
    m = dataclasses.replace(m, rti=m.rti if a.rti is None else a.rti, fast_sls_rti_steps=m.fast_sls_rti_steps if a.rti_steps is None else a.rti_steps)
    if a.sls_converge:
        m = dataclasses.replace(m, fast_sls_rti_steps=None)
    N = a.N or (10 if a.model == "pendulum" else 20)
    steps = a.steps or m.extra.get("sim_steps", 30)
    B = a.batch
    x0 = np.asarray(m.extra["x0"] if "x0" in m.extra else m.x_ref + 0.02 * (m.x_ub - m.x_lb), dtype=float)
    cont = 2 if a.model == "rocket" else 1
    seeds, warm_seeds = np.arange(B), np.arange(B, B + a.warm_batch)      # disjoint
    paths = {
        "a": lambda s: _run_slice(m, N, s, steps, x0, 0, True, True, cont, budget_ms=0),
        "b": lambda s: run_monte_carlo(m, N, s, steps, x0, solve_nominal=True, continuation=cont, budget_ms=0, slices=3),
        "c": lambda s: _run_slice(m, N, s, steps, x0, 0, True, True, cont, persistent=True, persistent_converge=a.sls_converge),
    }
    res, outs = {}, {}
    for p in a.paths:
        paths[p](warm_seeds)
        ts = []
        for _ in range(max(1, a.repeats)):
            t0 = time.perf_counter()
            outs[p] = paths[p](seeds)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = np.array(ts)
        res[p] = dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), ms_per_mpc_step=float(np.median(ts) / steps))
    line = dict(model=a.model, N=N, batch=B, steps=steps, rti=m.rti, rti_steps=m.fast_sls_rti_steps, repeats=a.repeats,
                run_on_device=res.get("a"), monte_carlo_3_slices=res.get("b"), persistent=res.get("c"))
    if "c" in outs:
        ls = outs["c"]["loop_stats"]
        line["loop_stats"] = ls
        line["wave_busy_frac"] = ls["busy_ms"] / max(1e-9, ls["waves"] * ls["launch_ms"])
        line["persistent_launch_ms_per_mpc_step"] = ls["launch_ms"] / steps
        line["solved"] = float(outs["c"]["success"].mean())
        line["scp_iterations_mean"] = float(outs["c"]["scp_iterations"].mean())
        if "sls_iterations" in outs["c"]:      # --sls-converge: the sweeps per MPC step, the spread the launch exploits
            it = outs["c"]["sls_iterations"]
            line["sls_iterations"] = dict(mean=float(it.mean()), max=int(it.max()), quantiles_0_50_90_99=[int(v) for v in np.quantile(it, [0.0, 0.5, 0.9, 0.99])],
                                          histogram={str(k): int(v) for k, v in zip(*np.unique(it, return_counts=True))})
    if "a" in outs and "c" in outs:
        same = all(np.array_equal(outs["a"][k], outs["c"][k], equal_nan=True) for k in KEYS)
        line["persistent_equals_run_on_device"] = bool(same)
    print(json.dumps(line), flush=True)
    if "a" in outs and "c" in outs:
        assert line["persistent_equals_run_on_device"], "the persistent launch and run_on_device disagree"


if __name__ == "__main__":
    main()

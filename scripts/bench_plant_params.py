#!/usr/bin/env python3
"""What the plant-parameter kernels cost: the persistent closed loop of a handle with plant parameters (k_cl_loop<M, 3>, the variant REF | PP of the
kernel: per MPC step one more RK4 step on the plant lane) against the variant without them (k_cl_loop<M, 1>), on identical inputs in one process.

All handles carry a one-row zero reference, so none takes the plain variant 0.  Three configurations, after a warm-up on a disjoint seed batch run in turn
`--repeats` times each:
  ref       no parameters (k_cl_loop<M, 1>)
  pp        the defaults set explicitly (k_cl_loop<M, 3>; a row equal to the model's constants takes the model's own step: model_error must be exactly zero; whether
            the outputs equal ref's bit for bit is reported as outputs_equal / differing_keys)
  pp_off    every parameter but the gimbal lengths off its default by a relative 1e-9 (k_cl_loop<M, 3> with BOTH RK4 steps on the plant lane: the cost of
            the feature; the closed loop is the same workload to nine digits)
Per run the duration of the persistent launch (HIP events around it, loop_stats.launch_ms) and the wall time of the whole run.  One JSON line:
medians and spreads (max - min).

    python scripts/bench_plant_params.py --model rocket --batch 4096 --steps 20
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robust_nonlinear_mpc_amd import ClosedLoopMPC, disturbance_stream, get_model, plant_param_defaults  # noqa: E402

KEYS = ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x", "backoff_trajectory_u", "success",
        "scp_iterations", "primal_infeasibility", "x0_violation", "qp_stats")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="rocket", choices=["pendulum", "quadrotor", "rocket"])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--x0-scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warm-batch", type=int, default=64)
    a = ap.parse_args()
    m = get_model(a.model)
    x0v = np.asarray(m.x_ref + a.x0_scale * (m.extra["x0"] - m.x_ref) if "x0" in m.extra else m.x_ref + 0.02 * (m.x_ub - m.x_lb), dtype=float)
    zero_ref = (np.zeros((1, m.nx)), np.zeros((1, m.nu)))
    cont = 2 if a.model == "rocket" else 1

    d = plant_param_defaults(m)
    off = d * np.where(np.arange(len(d)) < min(len(d), 8), 1.0 + 1e-9, 1.0)
    params = dict(ref=None, pp=d, pp_off=off)

    def run(seeds, cfg):
        B = len(seeds)
        W = np.stack([disturbance_stream(s, a.steps, m.nx) for s in seeds], axis=1)
        t0 = time.perf_counter()
        cl = ClosedLoopMPC(m, a.N, B, reference=zero_ref, plant_params=params[cfg])
        cl.f.opts.time_kernels = 1
        out = cl.run_decoupled(np.tile(x0v, (B, 1)), a.steps, W, solve_nominal=True, continuation=cont)
        cl.close()
        return out, (time.perf_counter() - t0) * 1e3

    seeds, warm = np.arange(a.batch), np.arange(a.batch, a.batch + a.warm_batch)
    for cfg in params:
        run(warm, cfg)
    launch, wall, outs, first = {c: [] for c in params}, {c: [] for c in params}, {}, {}
    for _ in range(max(1, a.repeats)):
        for cfg in params:
            outs[cfg], t = run(seeds, cfg)
            first.setdefault(cfg, outs[cfg])
            launch[cfg].append(outs[cfg]["loop_stats"]["launch_ms"])
            wall[cfg].append(t)

    def stat(v):
        v = np.array(v)
        return dict(median_ms=float(np.median(v)), spread_ms=float(v.max() - v.min()), runs_ms=[float(x) for x in v])
    differing = [k for k in KEYS if not np.array_equal(outs["ref"][k], outs["pp"][k], equal_nan=True)]
    unrepeatable = [k for k in KEYS if not np.array_equal(outs["ref"][k], first["ref"][k], equal_nan=True)]      # the same configuration, first run against last
    same = not differing
    line = dict(model=a.model, N=a.N, batch=a.batch, steps=a.steps, repeats=a.repeats, solved=float(outs["pp"]["success"].mean()),
                launch={c: stat(launch[c]) for c in params}, wall={c: stat(wall[c]) for c in params},
                launch_ms_per_mpc_step={c: float(np.median(launch[c]) / a.steps) for c in params},
                model_error_is_zero=bool(not outs["pp"]["model_error"].any()), outputs_equal=bool(same), differing_keys=differing, ref_keys_differing_between_repeats=unrepeatable,
                pp_off_largest_model_error=float(np.abs(outs["pp_off"]["model_error"]).max()), pp_off_solved=float(outs["pp_off"]["success"].mean()))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

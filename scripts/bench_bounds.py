#!/usr/bin/env python3
"""What the bounds kernels cost: the persistent closed loop of a handle with bounds (the variants with the BND bit of k_cl_loop<M, VAR>, VAR = 5 and 7: the window's rows in the
linearisation and the terminal tightened row read from the bounds buffer; variant 5 also subtracts the one-row zero reference of a handle that has
none) against the variant the same handle ran without them, on identical inputs in one process.  The bounds are the model's box repeated, so the
work per QP is the same.

Four configurations, after a warm-up on a disjoint seed batch run in turn `--repeats` times each:
  plain     nothing set (variant 0)
  bnd       the model's box as T = steps + N + 1 per-instance rows (variant 5 = REF | BND: reference + bounds, with the zero reference; the model's plant step)
  v2        a one-row zero reference and plant parameters 1e-9 off the defaults (variant 3 = REF | PP)
  v2_bnd    the same with the bounds (variant 7 = REF | PP | BND: reference + plant parameters + bounds)
Per run the duration of the persistent launch (HIP events around it, loop_stats.launch_ms).  One JSON line: medians and spreads (max - min), and
whether bnd / v2_bnd give the bits of plain / v2.

    python scripts/bench_bounds.py --model rocket --batch 4096 --steps 20
"""
import argparse
import json
import os
import sys

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
    T = a.steps + a.N + 1
    cfgs = dict(plain=dict(), bnd=dict(bounds=True), v2=dict(reference=zero_ref, plant_params=off), v2_bnd=dict(reference=zero_ref, plant_params=off, bounds=True))

    def run(seeds, cfg):
        B = len(seeds)
        W = np.stack([disturbance_stream(s, a.steps, m.nx) for s in seeds], axis=1)
        kw = dict(cfgs[cfg])
        if kw.pop("bounds", False):
            kw["bounds"] = (np.tile(m.g, (B, T, 1)), np.tile(m.gf, (B, T, 1)))
        cl = ClosedLoopMPC(m, a.N, B, **kw)
        cl.f.opts.time_kernels = 1
        out = cl.run_decoupled(np.tile(x0v, (B, 1)), a.steps, W, solve_nominal=True, continuation=cont)
        cl.close()
        return out

    seeds, warm = np.arange(a.batch), np.arange(a.batch, a.batch + a.warm_batch)
    for cfg in cfgs:
        run(warm, cfg)
    launch, outs = {c: [] for c in cfgs}, {}
    for _ in range(max(1, a.repeats)):
        for cfg in cfgs:
            outs[cfg] = run(seeds, cfg)
            launch[cfg].append(outs[cfg]["loop_stats"]["launch_ms"])

    def stat(v):
        v = np.array(v)
        return dict(median_ms=float(np.median(v)), spread_ms=float(v.max() - v.min()), runs_ms=[float(x) for x in v])

    def differing(x, y):
        return [k for k in KEYS if not np.array_equal(outs[x][k], outs[y][k], equal_nan=True)]
    line = dict(model=a.model, N=a.N, batch=a.batch, steps=a.steps, repeats=a.repeats, solved=float(outs["bnd"]["success"].mean()),
                launch={c: stat(launch[c]) for c in cfgs}, launch_ms_per_mpc_step={c: float(np.median(launch[c]) / a.steps) for c in cfgs},
                bnd_keys_differing_from_plain=differing("bnd", "plain"), v2_bnd_keys_differing_from_v2=differing("v2_bnd", "v2"),
                smallest_constraint_margin=float(outs["bnd"]["constraint_margin"].min()))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

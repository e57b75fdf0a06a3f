#!/usr/bin/env python3
"""Closed-loop robust MPC of the rockETH model for a batch of disturbance seeds on one MI355X -- the batched counterpart of the
reference's expe/main_rocket_robust_closed_loop.py `generate()` (same weights, E, x0, rti settings, 30 steps, seed-s noise streams).

    python examples/rocket_closed_loop.py --seeds 64 --steps 30 [--N 15] [--out results/]

The reference starts from an IPOPT nominal trajectory (SCP_SLS.solve_nominal_trajectory); here `--init sqp` (default) solves the same
nominal NLP on the GPU (slsqp_nominal_solve, trust-region SCP from a hover roll-out) and `--init rollout` uses the bare roll-out.
`--x0-scale s` starts from x_ref + s (x0_script - x_ref); the script's own x0 (s = 1, the default) needs the initial-state continuation
(`--continuation 2`, default).
`--plant-scale NAME=FACTOR` (repeatable) and `--plant-spread PCT` make the TRUE plant differ from the controller's model: a rocket that is heavier,
a servo that is slower, every parameter of seed s uniform within +-PCT % of its default.  The run then reports how often the model error plus the
noise left the disturbance box the tubes were designed for (`disturbance_used` > 1) and the constraint violations of the measured states.
`--solve-every M` runs the controller at 1/M of the plant's rate: a solve at steps 0, M, 2M, ..., the tube's feedback policy in between; with
`--persistent 1` the hold steps run inside the persistent launch (one launch for the whole loop), without it the loop is stepped.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robust_nonlinear_mpc_amd import get_model, plant_param_names, run_monte_carlo  # noqa: E402
from robust_nonlinear_mpc_amd._plant_cli import parse_plant_scale, sample_plant_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--N", type=int, default=15)          # the script's default horizon (main_rocket...:63)
    ap.add_argument("--x0-scale", type=float, default=1.0)
    ap.add_argument("--init", default="sqp", choices=["sqp", "rollout"])
    ap.add_argument("--continuation", type=int, default=2, help="stages of the initial-state continuation of the nominal NLP (far-away x0)")
    ap.add_argument("--slices", type=int, default=3, help="independent slices (own stream + host thread) the seeds are cut into")
    ap.add_argument("--round-budget-ms", type=float, default=None, help="run the loop through slsqp_cl_run: instances advance independently, rounds of this length")
    ap.add_argument("--x0-box-tol", type=float, default=0.0, help="how far the measured state may lie outside its own stage-0 box before a step is refused "
                    "(0: strict; 1e-3: what the reference's OSQP settings let through; inf: never)")
    ap.add_argument("--plant-scale", action="append", default=[], metavar="NAME=FACTOR",
                    help="the TRUE plant's parameter NAME is FACTOR x the controller's value, for every seed (repeatable), e.g. mass=1.15")
    ap.add_argument("--plant-spread", type=float, default=None, metavar="PCT",
                    help="every parameter of the true plant of seed s uniform within +-PCT %% of its default, drawn from a generator seeded with s (gimbal lengths excluded)")
    ap.add_argument("--solve-every", type=int, default=1, metavar="M",
                    help="the controller solves at steps 0, M, 2M, ... and holds its plan in between, the tube's feedback policy acting on the measured state (1 <= M <= N)")
    ap.add_argument("--persistent", type=int, default=None, choices=(0, 1), metavar="0|1",
                    help="1: the persistent launch wherever the setting allows it, --solve-every M > 1 included; 0: never; default: the plant's default, and a stepped loop for M > 1")
    ap.add_argument("--hold-trigger", type=float, default=None, metavar="THETA",
                    help="with --persistent 1 and --solve-every M > 1: a seed's controller holds while its measured state stays inside THETA x the tube of its plan "
                    "and solves when it does not, or after M steps at the latest")
    ap.add_argument("--plan-fallback", action="store_true",
                    help="a step that applies no freshly certified plan (a failed solve, a hold step) runs the tube policy of the seed's last plan that succeeded")
    ap.add_argument("--adversary", default="off", choices=["off", "nearest_bound", "away_from_target"],
                    help="the disturbance of every plant step is decided on the device from the seed's measured state: every state pushed towards the nearer "
                    "side of its box, or away from the origin; off: the seed's uniform stream")
    ap.add_argument("--adversary-amp", type=float, default=1.0, metavar="AMP",
                    help="size of the adversary's samples (1: the vertices of the box the tubes are computed for; above 1: outside it)")
    ap.add_argument("--meas-noise", type=float, default=None, metavar="AMP",
                    help="every seed's controller is given x_plant + AMP E[0] v, v a uniform unit sample per step, while the plant steps from x_plant "
                    "(1: the set the tubes' stage-0 column assumes); the printed states are then the true ones")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m = get_model("rocket")
    try:
        scale = parse_plant_scale(a.plant_scale)
        P = sample_plant_params(m, np.arange(a.seeds), a.plant_spread or 0.0, scale) if (scale or a.plant_spread is not None) else None
    except ValueError as e:
        ap.error(f"{e} (parameters: {', '.join(plant_param_names(m))})")
    x0 = m.x_ref + a.x0_scale * (m.extra["x0"] - m.x_ref)
    t0 = time.perf_counter()
    r = run_monte_carlo(m, a.N, np.arange(a.seeds), a.steps, x0, solve_nominal=(a.init == "sqp"), slices=a.slices, continuation=a.continuation,
                        budget_ms=a.round_budget_ms, x0_box_tol=a.x0_box_tol, plant_params=P, solve_every=a.solve_every,
                        persistent=None if a.persistent is None else bool(a.persistent), hold_trigger=a.hold_trigger, plan_fallback=a.plan_fallback,
                        adversary=None if a.adversary == "off" else a.adversary, adversary_amp=a.adversary_amp, meas_noise=a.meas_noise)
    dt = time.perf_counter() - t0
    ok = r["success"]
    if "nlp_status" in r:
        print(f"nominal NLP: status counts {np.bincount(r['nlp_status'], minlength=3).tolist()} (0 KKT point, 1 max QPs, 2 failed); "
              f"accepted steps mean {r['nlp_iterations'].mean():.1f}")
    print(f"{a.seeds} seeds x {a.steps} MPC steps (N={a.N}) in {dt:.2f} s; solved steps: {ok.mean():.3f}; "
          f"final |pos| mean {np.linalg.norm(r['state_trajectory'][:, :3, -1], axis=1).mean():.3f} "
          f"(start {np.linalg.norm(x0[:3]):.3f}); largest stage-0 violation of the measured state {r['x0_violation'].max():.2e}; QP {r['t_qp'].sum():.1f} ms, Riccati sweeps {r['t_riccati'].sum():.1f} ms")
    if a.solve_every > 1:
        held = r["hold_index"] > 0
        X = r["state_trajectory"]
        viol = np.maximum(X - m.x_ub[None, :, None], m.x_lb[None, :, None] - X).max(axis=1)
        print(f"solve every {a.solve_every} steps: {held.mean():.3f} of the steps held, the tube policy ran on {r['hold_policy'][held].mean():.3f} of them; "
              f"measured states outside the state box: {np.mean(viol > 0):.4f} of the steps")
    if "plan_age" in r:
        pol = r["hold_policy"]
        print(f"plan fallback: {np.mean(pol == 2):.4f} of the steps were failed solves that ran the last certified plan's policy (plan age there: median "
              f"{np.median(r['plan_age'][pol == 2]) if np.any(pol == 2) else 0:g}); failed solves left with the nominal input: {np.mean((r['hold_index'] == 0) & ~ok & (pol == 0)):.4f}")
    if "solve_trigger" in r:
        by = [float(np.mean(r["solve_trigger"] == c)) for c in (1, 2, 3)]
        print(f"hold trigger {a.hold_trigger:g}: steps solved on schedule {by[0]:.3f}, because the state left {a.hold_trigger:g} x tube {by[1]:.3f}, after a failed solve {by[2]:.3f}")
    if "measured_trajectory" in r:
        X = r["state_trajectory"]      # (the true states)
        viol = np.maximum(X - m.x_ub[None, :, None], m.x_lb[None, :, None] - X).max(axis=1)
        print(f"measurement noise amp {a.meas_noise:g}: largest |x_meas - x_plant| {np.abs(r['measured_trajectory'] - X).max():.3e}; true states outside the "
              f"state box {np.mean(viol > 0):.4f} of the steps; first QPs refused at x0 {np.mean(r['x0_violation'][:, :, 0] > max(1e-9, a.x0_box_tol)):.4f}")
    if "w_applied" in r:
        X = r["state_trajectory"]
        inside = np.all((X <= m.x_ub[None, :, None]) & (X >= m.x_lb[None, :, None]), axis=1)
        print(f"adversary {a.adversary} (amp {a.adversary_amp:g}): measured states inside the state box {inside.mean():.4f} of the steps; "
              f"largest disturbance_used {np.nanmax(r['disturbance_used']):.2f}")
    if P is not None:
        X = r["state_trajectory"]      # (seeds, nx, steps): the measured states
        viol = np.maximum(X - m.x_ub[None, :, None], m.x_lb[None, :, None] - X).max(axis=1)
        print(f"measured states outside the state box: {np.mean(viol > 0):.4f} of the steps, largest violation {max(viol.max(), 0.0):.3e}")
        du = r["disturbance_used"]
        print(f"plant mismatch (spread {a.plant_spread or 0.0:g} %, scale {scale or {}}): steps with disturbance_used > 1: {np.mean(du > 1.0):.4f}; "
              f"median {np.nanmedian(du):.2f}, largest {np.nanmax(du):.2f}")
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        from robust_nonlinear_mpc_amd import ClosedLoopMPC
        cl = ClosedLoopMPC(m, a.N, 1)
        cl.save_npz(os.path.join(a.out, "rockETH_robust_closed_loop_seed0.npz"), r, 0)
        cl.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Batched counterpart of the reference's three closed-loop scripts (expe/main_pendulum_robust_closed_loop.py,
main_quadrotor_robust_closed_loop.py, main_rocket_robust_closed_loop.py) on one MI355X: same weights, E, regularisers, rti /
fast_sls_rti_steps, step counts and (rocket) seed-s disturbance streams; B independent runs at once.

    python examples/closed_loop.py --model pendulum  [--runs 256]          # x0 = [0.5, 0.5, 0, 0], 60 steps, no noise (main_pendulum...:27-60,96)
    python examples/closed_loop.py --model quadrotor [--runs 256]          # random x0 around hover (the script's x0 is unseeded), 30 steps
    python examples/closed_loop.py --model rocket    [--runs 256] [--x0-scale 0.3]
    ... --persistent 1                                                     # the same loop as ONE persistent launch (same bits)
    ... --reference neutral | figure8                                      # track the plant's neutral point / a figure of eight in x, y
    ... --plant-scale mass=1.15 --plant-spread 10                          # a true plant that differs from the controller's model (see --help)
    ... --model quadrotor --bound 5=-1.2:inf@3                             # a box that changes during the run: descent rate >= -1.2 from step 3 on
    ... --solve-every 3                                                    # solve at steps 0, 3, 6, ...; the tube policy of the last solve acts in between
    ... --model rocket --persistent 1 --solve-every 5 --hold-trigger 0.75  # solve when the state leaves 0.75 x the plan's tube, or after 5 steps
    ... --persistent 1 --fast-sls-steps 0                                  # fast-SLS converge mode, every run iterating at its own pace in the one launch

The first nominal comes from the GPU initialiser (slsqp_nominal_solve) in place of IPOPT."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robust_nonlinear_mpc_amd import ClosedLoopMPC, box_bounds, disturbance_stream, get_model, meas_noise_table, measurement_stream, plant_param_names  # noqa: E402
from robust_nonlinear_mpc_amd._plant_cli import parse_plant_scale, sample_plant_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="pendulum", choices=["pendulum", "quadrotor", "rocket"])
    ap.add_argument("--runs", type=int, default=256)
    ap.add_argument("--N", type=int, default=None)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--x0-scale", type=float, default=0.3, help="rocket: x0 = x_ref + s (x0_script - x_ref); quadrotor: spread around hover")
    ap.add_argument("--persistent", type=int, default=0, choices=[0, 1],
                    help="1: the whole loop as one persistent launch (slsqp_cl_run / slsqp_cl_run_scp: instances advance independently, same bits); 0: one slsqp_cl_step per step")
    ap.add_argument("--x0-box-tol", type=float, default=0.0, help="how far the measured state may lie outside its own stage-0 box before a step is refused "
                    "(0: strict; 1e-3: what the reference's OSQP settings let through; inf: never)")
    ap.add_argument("--solve-waves", type=int, default=1, choices=[1, 2, 4, 8], help="waves per instance of the QP solves (above 1: the multi-wave kernel, for a few runs; "
                    "the loop then runs step by step)")
    ap.add_argument("--reference", default="none", choices=["none", "neutral", "figure8"],
                    help="what the loop tracks: none = the cost around the origin of the raw state (the scripts); neutral = the setpoint (x_ref, u_ref); "
                    "figure8 = x = 0.3 sin 2t, y = 0.3 (1 - cos 2t), z constant, the rest the neutral point (plants with a position: quadrotor, rocket)")
    ap.add_argument("--plant-scale", action="append", default=[], metavar="NAME=FACTOR",
                    help="the TRUE plant's parameter NAME is FACTOR x the controller's value, for every run (repeatable; names: plant_param_names(model))")
    ap.add_argument("--plant-spread", type=float, default=None, metavar="PCT",
                    help="every parameter of the true plant of run s uniform within +-PCT %% of its default, drawn from a generator seeded with s (gimbal lengths excluded)")
    ap.add_argument("--bound", action="append", default=[], metavar="IDX=LO:HI[@ROW]",
                    help="component IDX of [x; u] is held to [LO, HI] from MPC step ROW on (default 0), inside the model's own box; inf / -inf: that side keeps "
                    "the model's bound (repeatable)")
    ap.add_argument("--solve-every", type=int, default=1, metavar="M",
                    help="the controller solves at steps 0, M, 2M, ... and holds its plan in between, the tube's feedback policy acting on the measured state "
                    "(1 <= M <= N; above 1 the loop runs step by step)")
    ap.add_argument("--hold-trigger", type=float, default=None, metavar="THETA",
                    help="with --persistent 1 and --solve-every M > 1 (rti = 1 with one fast-SLS step: the rocket): an instance holds while its measured state stays "
                    "inside THETA x the tube of its plan and solves when it does not, or after M steps at the latest")
    ap.add_argument("--plan-fallback", action="store_true",
                    help="a step that applies no freshly certified plan (a failed solve, a hold step) runs the tube policy of the run's last plan that succeeded")
    ap.add_argument("--fast-sls-steps", type=int, default=None, metavar="K",
                    help="fast-SLS steps per solve instead of the script's value; 0: converge mode, every solve iterates until its step is below the tolerance "
                    "(fast_SLS.solve's default) -- with --persistent 1 inside the one launch, every run at its own pace")
    ap.add_argument("--adversary", default="off", choices=["off", "nearest_bound", "away_from_target"],
                    help="the disturbance of every plant step is decided on the device from the measured state: every state pushed towards the nearer side of "
                    "its box, or away from the reference (origin); off: the run's own samples")
    ap.add_argument("--adversary-amp", type=float, default=1.0, metavar="AMP",
                    help="size of the adversary's samples (1: the vertices of the box the tubes are computed for; above 1: outside it)")
    ap.add_argument("--meas-noise", type=float, default=None, metavar="AMP",
                    help="the controller is given x_plant + AMP E[0] v, v a uniform unit sample per run and step, while the plant steps from x_plant "
                    "(1: the set the tubes' stage-0 column assumes); the printed states are then the true ones")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m = get_model(a.model)
    try:
        scale = parse_plant_scale(a.plant_scale)
        P = sample_plant_params(m, np.arange(a.runs), a.plant_spread or 0.0, scale) if (scale or a.plant_spread is not None) else None
    except ValueError as e:
        ap.error(f"{e} (parameters of {a.model}: {', '.join(plant_param_names(m))})")
    N = a.N or 15                                                            # the scripts' default horizon (main_*_robust_closed_loop.py: N = 15)
    steps = a.steps or m.extra.get("sim_steps", 30)
    B = a.runs
    rng = np.random.default_rng(0)
    if a.model == "pendulum":
        x0 = np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.2 * rng.uniform(-1, 1, (B, 1)))
        x0[0] = m.extra["x0"]                                                # run 0 is the script's own
        W = None
    elif a.model == "quadrotor":
        D = np.array([2.0] * 3 + [1.0] * 3 + [0.0, 0.1, 0.1, 0.1] + [0.5] * 3)
        x0 = m.x_ref + a.x0_scale * D * rng.uniform(-1, 1, (B, m.nx))
        x0[:, 6:10] /= np.linalg.norm(x0[:, 6:10], axis=1, keepdims=True)
        W = None
    else:
        x0 = np.tile(m.x_ref + a.x0_scale * (m.extra["x0"] - m.x_ref), (B, 1))
        W = np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)   # seed 0 = the script's stream
    Xref = None
    if a.reference == "neutral":
        Xref, Uref = np.asarray(m.x_ref, dtype=float)[None, :], np.asarray(m.u_ref, dtype=float)[None, :]
    elif a.reference == "figure8":
        if a.model == "pendulum":
            ap.error("--reference figure8 needs a plant with a position in space (quadrotor, rocket)")
        T = steps + N + 1
        t = 0.05 * np.arange(T)                                              # row t of the reference = MPC step t (RK4 step 0.05 s)
        Xref = np.tile(np.asarray(m.x_ref, dtype=float), (T, 1))
        Xref[:, 0], Xref[:, 1] = 0.3 * np.sin(2.0 * t), 0.3 * (1.0 - np.cos(2.0 * t))
        Uref = np.tile(np.asarray(m.u_ref, dtype=float), (T, 1))
    bounds = None
    if a.bound:
        Tb = steps + N + 1
        spec = {}
        for item in a.bound:
            try:
                idx, rest = item.split("=", 1)
                rng_, _, row = rest.partition("@")
                lo_s, hi_s = rng_.split(":", 1)
                idx, lo_v, hi_v, row = int(idx), float(lo_s), float(hi_s), int(row or 0)
            except ValueError:
                ap.error(f"--bound {item!r}: expected IDX=LO:HI[@ROW]")
            on = np.arange(Tb) >= row
            spec[idx] = (np.where(on, lo_v, -np.inf), np.where(on, hi_v, np.inf))      # (before ROW and on an infinite side: the model's own bound)
        try:
            bounds = box_bounds(m, Tb, spec)
        except ValueError as e:
            ap.error(str(e))
    cl = ClosedLoopMPC(m, N, B, x0_box_tol=a.x0_box_tol, solve_waves=a.solve_waves, reference=None if Xref is None else (Xref, Uref), plant_params=P, bounds=bounds,
                       solve_every=a.solve_every, plan_fallback=a.plan_fallback, adversary=None if a.adversary == "off" else a.adversary, adversary_amp=a.adversary_amp,
                       meas_noise=None if a.meas_noise is None else meas_noise_table(m, np.stack([measurement_stream(s, steps + 1, m.nw) for s in range(B)]), a.meas_noise))
    if a.fast_sls_steps is not None:
        cl.f.set_rti_steps(a.fast_sls_steps)      # (0: converge mode)
    t0 = time.perf_counter()
    run = cl.run_decoupled if a.persistent else cl.run_on_device
    kw = {} if a.hold_trigger is None else dict(hold_trigger=a.hold_trigger, **(dict(persistent_hold=True) if a.persistent else {}))
    if a.persistent and cl.f.opts.rti_steps <= 0:
        kw["persistent_converge"] = True
    out = run(x0, steps, W, solve_nominal=True, continuation=2 if a.model == "rocket" else 1, **kw)
    dt = time.perf_counter() - t0
    dist0 = np.linalg.norm(out["state_trajectory"][:, :, 0] - m.x_ref, axis=1).mean()
    dist1 = np.linalg.norm(out["state_trajectory"][:, :, -1] - m.x_ref, axis=1).mean()
    print(f"{a.model}: {B} runs x {steps} MPC steps (N={N}, rti={cl.rti}) in {dt:.2f} s; nominal NLP solved for {np.mean(cl.nlp_status == 0):.3f}; "
          f"MPC steps solved {out['success'].mean():.3f}; mean |x - x_ref| {dist0:.3f} -> {dist1:.3f}; QP {out['t_qp'].sum():.0f} ms, sweeps {out['t_riccati'].sum():.0f} ms")
    if "sls_iterations" in out:
        it = out["sls_iterations"]
        print(f"fast-SLS converge mode in the persistent launch: sweeps per MPC step min {it.min()} / median {int(np.median(it))} / max {it.max()}; "
              f"waves busy {out['loop_stats']['busy_ms'] / max(out['loop_stats']['waves'] * out['loop_stats']['launch_ms'], 1e-9):.2f} of the launch")
    if "plan_age" in out:
        pol = out["hold_policy"]
        print(f"plan fallback: {np.mean(pol == 2):.4f} of the steps were failed solves that ran the last certified plan's policy; "
              f"failed solves left with the nominal input: {np.mean((out['hold_index'] == 0) & ~out['success'] & (pol == 0)):.4f}")
    if a.solve_every > 1:
        held = out["hold_index"] > 0
        print(f"solve every {a.solve_every} steps: {held.mean():.3f} of the steps held; the tube policy ran on {out['hold_policy'][held].mean():.3f} of them "
              f"(the rest had no valid plan and applied the nominal input)")
    if "solve_trigger" in out:
        by = [float(np.mean(out["solve_trigger"] == c)) for c in (1, 2, 3)]
        print(f"hold trigger {a.hold_trigger:g}: steps solved on schedule {by[0]:.3f}, because the state left {a.hold_trigger:g} x tube {by[1]:.3f}, after a failed solve {by[2]:.3f}")
    if P is not None:
        du = out["disturbance_used"]
        print(f"plant mismatch: steps with disturbance_used > 1 (model error + noise outside the box the tubes assume): {np.mean(du > 1.0):.3f}; "
              f"largest {np.nanmax(du):.2f}; largest |model error| {np.abs(out['model_error']).max():.3e}")
    if "measured_trajectory" in out:
        print(f"measurement noise amp {a.meas_noise:g}: MPC steps solved {out['success'].mean():.3f}; largest |x_meas - x_plant| "
              f"{np.abs(out['measured_trajectory'] - out['state_trajectory']).max():.3e}; largest stage-0 violation of the measurement {out['x0_violation'].max():.2e}")
    if "w_applied" in out:
        X = out["state_trajectory"]
        inside = np.all((X <= m.x_ub[None, :, None]) & (X >= m.x_lb[None, :, None]), axis=1)
        print(f"adversary {a.adversary} (amp {a.adversary_amp:g}): MPC steps solved {out['success'].mean():.3f}; measured states inside the model's state box "
              f"{inside.mean():.4f} of the steps; largest disturbance_used {np.nanmax(out['disturbance_used']):.2f}")
    if bounds is not None:
        print(f"bounds {' '.join(a.bound)}: MPC steps solved {out['success'].mean():.3f}; smallest constraint_margin {out['constraint_margin'].min():.3e} "
              f"(negative: the measured state or applied input left the box in force at that step)")
    if Xref is not None:
        rows = np.minimum(np.arange(steps), len(Xref) - 1)
        err = np.linalg.norm(out["state_trajectory"].transpose(0, 2, 1) - Xref[rows][None], axis=2).mean(axis=0)      # (steps,)
        print(f"reference {a.reference}: mean distance of the measured state to the reference {err[0]:.3f} at the first step -> {err[-1]:.3f} at the last")
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        cl.save_npz(os.path.join(a.out, f"{a.model}_robust_closed_loop_run0.npz"), out, 0)
    cl.close()


if __name__ == "__main__":
    main()

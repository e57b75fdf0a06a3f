#!/usr/bin/env python3
"""What holding an MPC solution costs and keeps: the rocket closed loop of bench.py (N = 20, the script's x0, seed-s noise streams) through
ClosedLoopMPC.run_on_device with a solve every M steps and the tube's feedback policy in between (slsqp_cl_hold_step).

    python scripts/bench_hold.py [--batch 4096] [--steps 30] [--M 1 2 3 5] [--reps 5] [--root DIR] [--persistent [--trigger THETA]] [--plant-spread PCT]

--persistent: the same loop as ONE persistent launch (ClosedLoopMPC.run_decoupled, for M > 1 with persistent_hold=True: the hold steps run inside the
launch); the timed span is then reset's return to the launch's end (the upload of the noise samples included), and the line also
holds `persistent`, `loop_stats` of the last run and `waves_busy` = busy_ms / (waves x launch's wall time), how busy the instance queue kept the waves.

--persistent --trigger THETA: event-triggered solves (run_decoupled's hold_trigger): an instance holds while its state stays
inside THETA x its tube and solves when it does not, or after M steps at the latest.  The line then also holds `trigger`, `solved_share` (the share of
instance-steps that solved) and `solved_by_reason` (its split: 1 scheduled, 2 the state left THETA x tube, 3 the last solve had failed), and the tube
quantiles are those of the logged `tube_ratio` over the instance-steps where it was evaluated.  THETA = inf is the fixed period.

Per M, one JSON line:
  ms_per_step        median over --reps runs of the wall time of the loop (first slsqp_cl_step / slsqp_cl_hold_step to the last one's return; the
                     reset before it and the read-back of the log after it are not timed) divided by the steps; `ms_per_step_runs` holds every run
  solved_ok          share of the solved steps that succeeded
  inside_box         share of all steps whose measured state lies inside the model's state box
  tube_ratio_max     largest |x_meas - z_k|_i / backoff_x[k]_i over the hold steps on which the policy ran (the tubes are row 2-norms of the response
                     to |w|_2 <= 1 while the samples are uniform in the box |w|_inf <= 1: a ratio above 1 is possible), with `tube_ratio_at` = where it
                     occurred (instance, step, hold index k, state component, deviation, back-off); tube_ratio_p50 / _p99 the quantiles of the
                     per-(instance, hold step) largest ratio and tube_exceeded the share of those above 1
The nominal trajectory of the first step is solved once (slsqp_nominal_solve) and handed to every run, so all runs of all M start from the same plan.
M = 1 does not name `solve_every` at all: with --root pointing at another checkout (with its library built) the same command measures that tree."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--M", type=int, nargs="+", default=[1, 2, 3, 5])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--persistent", action="store_true", help="one persistent launch per run instead of one launch sequence per step")
    ap.add_argument("--trigger", type=float, default=None, help="theta of the event-triggered schedule (with --persistent and M > 1; inf or absent: the fixed period)")
    ap.add_argument("--fallback", action="store_true", help="plan fallback on (DESIGN.md section 22): a failed solve and every hold step run the policy of the last plan that succeeded")
    ap.add_argument("--plant-spread", type=float, default=None, metavar="PCT",
                    help="every instance's true plant with its parameters within +-PCT %% of their defaults (ClosedLoopMPC's plant_params): the stepped loop then "
                    "launches the plant-parameter kernels, k_cl_shift_plant_pp and k_cl_hold<., true>")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package is measured")
    a = ap.parse_args()
    triggered = a.trigger is not None and a.trigger < float("inf")
    if triggered and not a.persistent:
        ap.error("--trigger needs --persistent: the event-triggered schedule runs in the persistent launch only")
    sys.path.insert(0, os.path.abspath(a.root))
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, disturbance_stream, get_model
    m = get_model("rocket")
    B, N, steps = a.batch, a.N, a.steps
    x0 = np.tile(np.asarray(m.extra["x0"], dtype=float), (B, 1))
    W = np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)
    cl = ClosedLoopMPC(m, N, B)
    cl.reset(x0, solve_nominal=True, continuation=2)
    X_nom, U_nom = cl.f.get("nominal_x", (N + 1, m.nx)), cl.f.get("nominal_u", (N, m.nu))
    nlp_ok = float(np.mean(cl.nlp_status == 0))
    cl.close()
    for M in a.M:
        kw = dict(plan_fallback=True) if a.fallback else {}      # (off: the option is not named at all, as solve_every for M = 1)
        if a.plant_spread is not None:
            from robust_nonlinear_mpc_amd._plant_cli import sample_plant_params
            kw["plant_params"] = sample_plant_params(m, np.arange(B), a.plant_spread)
        cl = ClosedLoopMPC(m, N, B, **kw) if M == 1 else ClosedLoopMPC(m, N, B, solve_every=M, **kw)
        mark = {}
        reset, log_result = cl.reset, cl._log_result

        def timed_reset(*args, **kw):
            r = reset(*args, **kw)
            mark["t0"] = time.perf_counter()
            return r

        def timed_log_result(*args, **kw):
            mark["t1"] = time.perf_counter()
            return log_result(*args, **kw)
        cl.reset, cl._log_result = timed_reset, timed_log_result
        runs, out = [], None
        for _ in range(a.reps + 1):      # (the first run warms the code objects and the allocator: not counted)
            if a.persistent:
                if M > 1 and triggered:
                    out = cl.run_decoupled(x0, steps, W, X_nom, U_nom, persistent_hold=True, hold_trigger=a.trigger)
                else:
                    out = cl.run_decoupled(x0, steps, W, X_nom, U_nom) if M == 1 else cl.run_decoupled(x0, steps, W, X_nom, U_nom, persistent_hold=True)
            else:
                out = cl.run_on_device(x0, steps, W, X_nom, U_nom)
            runs.append(1e3 * (mark["t1"] - mark["t0"]) / steps)
        cl.close()
        runs = runs[1:]
        X = out["state_trajectory"]                                     # (B, nx, steps): the measured state every step started from
        inside = np.all((X <= m.x_ub[None, :, None]) & (X >= m.x_lb[None, :, None]), axis=1)
        solved = np.arange(steps) % M == 0
        rec = dict(M=M, plant_spread=a.plant_spread, batch=B, N=N, steps=steps, nlp_ok=nlp_ok, ms_per_step=float(np.median(runs)), ms_per_step_runs=[round(r, 4) for r in runs],
                   solved_ok=float(out["success"][:, solved].mean()), inside_box=float(inside.mean()))
        if "solve_trigger" in out:      # every instance on its own schedule
            did = out["hold_index"] == 0
            trig, r = out["solve_trigger"], out["tube_ratio"]
            ev = np.zeros_like(did)
            ev[:, 1:] = out["success"][:, :-1]
            per = r[ev]
            rec.update(trigger=a.trigger, solved_ok=float(out["success"][did].mean()), solved_share=float(did.mean()),
                       solved_by_reason={str(c): float(np.mean(trig == c)) for c in (1, 2, 3)}, policy_ran=float(out["hold_policy"][~did].mean()) if (~did).any() else 0.0,
                       inside_box_hold_steps=float(inside[~did].mean()) if (~did).any() else 0.0, inside_box_solved_steps=float(inside[did].mean()),
                       tube_nonfinite=int(np.sum(~np.isfinite(per))))
            per = per[np.isfinite(per)]
            rec.update(tube_ratio_max=float(per.max()), tube_ratio_p50=float(np.median(per)), tube_ratio_p99=float(np.quantile(per, 0.99)), tube_exceeded=float(np.mean(per > 1.0)))
        if "plan_age" in out:      # plan fallback: what the steps without a fresh plan did, and the tube of the backup on the failed solves that ran its policy
            pol, age = out["hold_policy"], out["plan_age"]
            fell = pol == 2
            rec.update(fallback=True, success_share=float(out["success"][out["hold_index"] == 0].mean()), policy2_share=float(fell.mean()),
                       policy0_share_unsolved=float(np.mean((pol == 0) & ~((out["hold_index"] == 0) & out["success"]))),
                       plan_age_at_fallback={str(k): int(np.sum(age[fell] == k)) for k in np.unique(age[fell])})
        if a.persistent:
            ls = out["loop_stats"]
            rec.update(persistent=True, loop_stats=ls, waves_busy=float(ls["busy_ms"] / max(1e-9, ls["waves"] * runs[-1] * steps)))
        if M > 1 and "solve_trigger" not in out:
            per, at = [], None
            for i in np.nonzero(~solved)[0]:
                k = i % M
                ran = np.nonzero(out["hold_policy"][:, i])[0]
                if not len(ran):
                    continue
                dev, bo = np.abs(X[ran, :, i] - out["nominal_trajectory_x"][ran, :, 0, i]), out["backoff_trajectory_x"][ran, :, k, i]
                r = dev / bo
                per.append(r.max(axis=1))      # (NaN / inf where the plant has diverged: counted below)
                r = np.where(np.isfinite(r), r, -1.0)
                if at is None or r.max() > at["ratio"]:
                    bi, c = np.unravel_index(np.argmax(r), r.shape)
                    at = dict(ratio=float(r[bi, c]), instance=int(ran[bi]), step=int(i), k=int(k), component=int(c), deviation=float(dev[bi, c]), backoff=float(bo[bi, c]))
            per = np.concatenate(per)
            rec["tube_nonfinite"] = int(np.sum(~np.isfinite(per)))      # (instance, hold step) pairs of a plant that has diverged to inf / NaN
            per = per[np.isfinite(per)]
            rec.update(tube_ratio_max=float(per.max()), tube_ratio_p50=float(np.median(per)), tube_ratio_p99=float(np.quantile(per, 0.99)),
                       tube_exceeded=float(np.mean(per > 1.0)), tube_ratio_at=at, policy_ran=float(out["hold_policy"][:, ~solved].mean()), inside_box_hold_steps=float(inside[:, ~solved].mean()),
                       inside_box_solved_steps=float(inside[:, solved].mean()))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

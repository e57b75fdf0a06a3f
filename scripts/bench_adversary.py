#!/usr/bin/env python3
"""What the tubes hold under a disturbance that reacts to the state: the rocket closed loop of bench.py (N = 20, the script's x0) as ONE persistent
launch (ClosedLoopMPC.run_decoupled), with the seeds' uniform noise streams against the state-feedback adversary (slsqp_cl_set_adversary, DESIGN.md
section 24) -- both policies at amp 0.5 and 1.0 -- for a solve at every step (M = 1) and a solve every third step with the tube policy in between
(M = 3, persistent_hold).

    python scripts/bench_adversary.py [--batch 4096] [--steps 30] [--N 20] [--M 1 3] [--amp 0.5 1.0] [--reps 5]

Per (M, disturbance), one JSON line:
  ms_per_step        median over --reps runs of the wall time from reset's return to the end of the launch (the upload of the samples included), per
                     closed-loop step; `ms_per_step_runs` holds every run (a first, uncounted run warms the code objects)
  solved_share       share of the solved steps that succeeded
  inside_box         share of all steps whose measured state lies inside the model's state box
  margin_min         smallest constraint_margin: the distance of measured state and applied input to the model's box, over all steps (negative: outside)
  tube_ratio_max     largest |x_meas(t + k) - z_k|_i / backoff_x[k]_i over the steps t that solved and succeeded, k = 1 (the next measured state against
                     the plan's stage 1) and, for M > 1, the hold steps k = 1 .. M - 1 on which the policy ran; tube_exceeded = share of those
                     (instance, step) pairs with a ratio above 1, tube_nonfinite = pairs of a plant that diverged
  disturbance_used   the largest |w|_inf the plant steps used (1 for amp = 1; the uniform streams stay below it)
The nominal trajectory of the first step is solved once and handed to every run, so all runs start from the same plan."""
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
    ap.add_argument("--M", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--amp", type=float, nargs="+", default=[0.5, 1.0])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, constraint_margin, disturbance_stream, get_model
    m = get_model("rocket")
    B, N, steps = a.batch, a.N, a.steps
    x0 = np.tile(np.asarray(m.extra["x0"], dtype=float), (B, 1))
    W = np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)
    cl = ClosedLoopMPC(m, N, B)
    cl.reset(x0, solve_nominal=True, continuation=2)
    X_nom, U_nom = cl.f.get("nominal_x", (N + 1, m.nx)), cl.f.get("nominal_u", (N, m.nu))
    nlp_ok = float(np.mean(cl.nlp_status == 0))
    cl.close()
    settings = [("noise", None, None)] + [(p, p, amp) for p in ("nearest_bound", "away_from_target") for amp in a.amp]
    for M in a.M:
        for label, policy, amp in settings:
            cl = ClosedLoopMPC(m, N, B) if policy is None else ClosedLoopMPC(m, N, B, adversary=policy, adversary_amp=amp)      # (off: the option is not named at all)
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
            for _ in range(a.reps + 1):
                out = cl.run_decoupled(x0, steps, W, X_nom, U_nom) if M == 1 else cl.run_decoupled(x0, steps, W, X_nom, U_nom, solve_every=M, persistent_hold=True)
                runs.append(1e3 * (mark["t1"] - mark["t0"]) / steps)
            cl.close()
            runs = runs[1:]
            X = out["state_trajectory"]                                     # (B, nx, steps)
            inside = np.all((X <= m.x_ub[None, :, None]) & (X >= m.x_lb[None, :, None]), axis=1)
            solved = np.arange(steps) % M == 0
            margin = constraint_margin(m, np.asarray(m.g, dtype=float)[None, :], X, out["input_trajectory"])
            nomx, bx = out["nominal_trajectory_x"], out["backoff_trajectory_x"]      # (B, nx, N + 1, steps)
            per = []
            for t in np.nonzero(solved)[0]:
                ok = out["success"][:, t]
                for k in ([1] if M == 1 else range(1, M)):      # M = 1: the next solve's measured state; M > 1: the hold steps of this solve
                    if t + k >= steps:
                        break
                    ran = ok if (M == 1 or "hold_policy" not in out) else ok & (out["hold_policy"][:, t + k] != 0)
                    if not ran.any():
                        continue
                    r = np.abs(X[ran, :, t + k] - nomx[ran, :, k, t]) / bx[ran, :, k, t]
                    per.append(r.max(axis=1))
            per = np.concatenate(per) if per else np.zeros(0)
            nonfinite = int(np.sum(~np.isfinite(per)))
            per = per[np.isfinite(per)]
            ls = out["loop_stats"]
            rec = dict(M=M, disturbance=label, amp=amp, batch=B, N=N, steps=steps, nlp_ok=nlp_ok, ms_per_step=float(np.median(runs)), ms_per_step_runs=[round(r, 4) for r in runs],
                       solved_share=float(out["success"][:, solved].mean()), inside_box=float(inside.mean()), margin_min=float(np.nanmin(margin)),
                       tube_ratio_max=float(per.max()) if len(per) else None, tube_ratio_p99=float(np.quantile(per, 0.99)) if len(per) else None,
                       tube_exceeded=float(np.mean(per > 1.0)) if len(per) else None, tube_nonfinite=nonfinite,
                       disturbance_used=float(np.nanmax(out["disturbance_used"])) if "disturbance_used" in out else float(np.abs(W).max()),
                       waves_busy=float(ls["busy_ms"] / max(1e-9, ls["waves"] * runs[-1] * steps)))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

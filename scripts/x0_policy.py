#!/usr/bin/env python3
"""What the x0 tolerance (slsqp_set_x0_box_tol) does to the rocket script's closed loop (script x0, N = 20, rti = 1, one fast-SLS step, seed-s
disturbance streams), on one MI355X:

    python scripts/x0_policy.py [--seeds 1024] [--steps 30] [--repeat 3]
        the Monte-Carlo under the three policies -- strict (0), X0_BOX_TOL_OSQP_DEFAULT, inf -- as ONE persistent launch each; per closed-loop step
        mpc_step_success_frac, QP solves executed, block solves per executed QP; per policy the launch's duration per step (median of --repeat runs).
        The tolerant policies run more QPs: a different workload per line, reported, not compared for speed.
    python scripts/x0_policy.py --record tests/golden/x0_violation_rocket_script.npz
        the strict 64-seed x 30-step loop of tests/test_gpu_parity.py's script-regime test; writes (seed, step, slot, violation, status) of all
        64 x 30 x 2 QPs and prints where today's status-2 solves lie relative to the constant and to 1e-2.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robust_nonlinear_mpc_amd import ClosedLoopMPC, X0_BOX_TOL_OSQP_DEFAULT, disturbance_stream, get_model  # noqa: E402


def run(m, N, seeds, steps, tol, timed=False):
    B = len(seeds)
    W = np.stack([disturbance_stream(s, steps, m.nx) for s in seeds], axis=1)
    cl = ClosedLoopMPC(m, N, B, x0_box_tol=tol)
    cl.f.opts.time_kernels = 1 if timed else 0
    out = cl.run_decoupled(np.tile(m.extra["x0"], (B, 1)), steps, W, solve_nominal=True, continuation=2)
    cl.close()
    return out


def split(viol, status, const):
    """today's status-2 solves: below the constant, between it and 1e-2, above"""
    v = viol[status == 2]
    return int((v <= const).sum()), int(((v > const) & (v <= 1e-2)).sum()), int((v > 1e-2).sum()), v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--record", default=None, metavar="NPZ")
    a = ap.parse_args()
    m = get_model("rocket")
    if a.record:
        S, steps = 64, 30
        out = run(m, a.N, np.arange(S), steps, 0.0)
        viol, st = out["x0_violation"], out["qp_stats"][..., 6]          # (S, steps, 2)
        seed, step, slot = np.meshgrid(np.arange(S), np.arange(steps), np.arange(2), indexing="ij")
        np.savez_compressed(a.record, seed=seed.ravel().astype(np.int16), step=step.ravel().astype(np.int16), slot=slot.ravel().astype(np.int8),
                            violation=viol.ravel(), status=st.ravel().astype(np.int8))
        for sl in (0, 1):
            lo, mid, hi, v = split(viol[:, :, sl], st[:, :, sl], X0_BOX_TOL_OSQP_DEFAULT)
            took = int((st[:, :, sl] != -1).sum())
            print(f"QP #{sl + 1}: {took} took part, {lo + mid + hi} status 2: {lo} <= {X0_BOX_TOL_OSQP_DEFAULT:g}, {mid} in ({X0_BOX_TOL_OSQP_DEFAULT:g}, 1e-2], {hi} > 1e-2; "
                  f"violation quantiles (min, 10 %, median, 90 %, max): {np.quantile(v, [0, 0.1, 0.5, 0.9, 1]) if v.size else None}")
        print(f"mpc_step_success_frac: all steps {out['success'].mean():.4f}, last step {out['success'][:, -1].mean():.4f}")
        per_seed = [(s, int(((viol[s] > 1e-9) & (viol[s] <= X0_BOX_TOL_OSQP_DEFAULT) & (st[s] == 2)).sum())) for s in range(S)]
        print("status-2 solves at or below the constant, per seed (seed, count):", [p for p in per_seed if p[1]])
        return
    seeds = np.arange(a.seeds)
    run(m, a.N, seeds[:64], 2, 0.0)          # (untimed: module load, first launches)
    for name, tol in (("strict", 0.0), (f"{X0_BOX_TOL_OSQP_DEFAULT:g}", X0_BOX_TOL_OSQP_DEFAULT), ("inf", float("inf"))):
        outs = [run(m, a.N, seeds, a.steps, tol, timed=True) for _ in range(max(1, a.repeat))]
        ms = sorted(o["loop_stats"]["launch_ms"] for o in outs)
        out = outs[0]
        st, bs = out["qp_stats"][..., 6], out["qp_stats"][..., 1]          # (S, steps, 2)
        ran = (st != -1) & (st != 2)
        lo, mid, hi, _ = split(out["x0_violation"], st, X0_BOX_TOL_OSQP_DEFAULT)
        print(f"policy {name}: {a.seeds} seeds x {a.steps} steps, persistent launch {ms[len(ms) // 2]:.1f} ms = {ms[len(ms) // 2] / a.steps:.3f} ms per step "
              f"(median of {len(ms)}; min {ms[0]:.1f}, max {ms[-1]:.1f}); success all steps {out['success'].mean():.4f}; QP solves executed {int(ran.sum())}; "
              f"block solves per executed QP {bs[ran].mean():.2f}; status 2: {lo + mid + hi} ({lo} / {mid} / {hi} below the constant / up to 1e-2 / above); "
              f"status 5: {int((st == 5).sum())}, status 1 / 3: {int(np.isin(st, (1, 3)).sum())}")
        print("  step  success_frac  qp_solves  block_solves_per_qp")
        for i in range(a.steps):
            r = ran[:, i]
            print(f"  {i:4d}  {out['success'][:, i].mean():12.4f}  {int(r.sum()):9d}  {bs[:, i][r].mean() if r.any() else float('nan'):19.2f}")


if __name__ == "__main__":
    main()

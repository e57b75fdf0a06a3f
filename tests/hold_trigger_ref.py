"""numpy restatement of the event-triggered hold schedule (csrc/cl_hold.hpp: tube_term, decide), for the tests.

An instance about to begin its closed-loop step s >= 1 holds (hold step k = k_prev + 1) while its measured state x stays inside the fraction theta of
the tube of its plan: r = max_i |x_i - z_i| / bo_i <= theta, z stage k of the plan, bo row k of the last solve's backoff_x.  It solves otherwise, or
when k reaches M, or when its last solve failed."""
import numpy as np

HOLD, SCHEDULED, TUBE, FAILED = 0, 1, 2, 3


def tube_ratio(x, z, bo):
    """max_i |x_i - z_i| / bo_i over the last axis, plain fp64.  bo_i = 0: 0 if x_i == z_i, else inf; a NaN term counts as inf."""
    x, z, bo = np.broadcast_arrays(np.asarray(x, dtype=float), np.asarray(z, dtype=float), np.asarray(bo, dtype=float))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.abs(x - z) / bo
    t = np.where(np.isnan(t), np.inf, t)
    t = np.where(bo == 0.0, np.where(x == z, 0.0, np.inf), t)
    return np.max(t, axis=-1) if t.shape[-1] else np.zeros(t.shape[:-1])


def decide(s, k_prev, M, plan_ok, r, theta):
    """The reason code of step s: 0 = hold step k_prev + 1, every other code a solve (1 scheduled, 3 the last solve failed, 2 the state left
    theta x tube), in this precedence.  r is read only where s >= 1 and plan_ok."""
    if s == 0 or k_prev + 1 >= M:
        return SCHEDULED
    if not plan_ok:
        return FAILED
    if not (r <= theta):
        return TUBE
    return HOLD


def schedule_from_log(result, M, theta):
    """(ratio, reason, hold_index), each (B, steps), recomputed from a result's own arrays: at step s, x = state_trajectory[..., s], z = stage 1 of
    step s - 1's logged nominal, bo = row k of step s - 1's logged backoff_x, plan_ok = step s - 1's success.  The ratio is 0 where it is not
    evaluated (s = 0, or no valid plan)."""
    X = np.asarray(result["state_trajectory"])            # (B, nx, steps)
    Z = np.asarray(result["nominal_trajectory_x"])        # (B, nx, N + 1, steps)
    BO = np.asarray(result["backoff_trajectory_x"])       # (B, nx, N + 1, steps)
    ok = np.asarray(result["success"]).astype(bool)       # (B, steps)
    B, _, steps = X.shape
    N = Z.shape[2] - 1
    ratio, reason, hold = np.zeros((B, steps)), np.zeros((B, steps), dtype=np.int32), np.zeros((B, steps), dtype=np.int32)
    for b in range(B):
        k_prev = 0
        for s in range(steps):
            r = 0.0
            if s >= 1 and ok[b, s - 1] and k_prev + 1 <= N:
                r = float(tube_ratio(X[b, :, s], Z[b, :, 1, s - 1], BO[b, :, k_prev + 1, s - 1]))
            code = decide(s, k_prev, M, s >= 1 and bool(ok[b, s - 1]), r, theta)
            ratio[b, s], reason[b, s] = r, code
            k_prev = k_prev + 1 if code == HOLD else 0
            hold[b, s] = k_prev
    return ratio, reason, hold

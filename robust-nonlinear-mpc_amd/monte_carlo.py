"""Closed-loop Monte-Carlo over disturbance seeds, sharded across ranks (BASELINE.json config 5).

Seed s reproduces the disturbance stream of the reference script for `np.random.seed(s)`
(expe/main_rocket_robust_closed_loop.py:30,180: w_t = 2*rand(nx) - 1 per closed-loop step; seed 0 is the script's own run).
Rank r owns the contiguous seed slice shard_range(S, r, world); the only collective is one all-gather of the trajectories.
"""
import os

import numpy as np

from .closed_loop import ClosedLoopMPC
from .sharding import gather_rows, shard_range


def disturbance_stream(seed, steps, nx):
    rs = np.random.RandomState(int(seed))
    return np.stack([2.0 * rs.rand(nx) - 1.0 for _ in range(steps)])


def measurement_stream(seed, rows, nw):
    """(rows, nw) unit sample in [-1,1] for the measurement noise of seed `seed`: a stream of its own (the seed and a fixed tag seed the generator), so
    disturbance_stream of the same seed is what it always was."""
    rs = np.random.RandomState([int(seed) & 0xFFFFFFFF, 0x6D656173])
    return 2.0 * rs.rand(int(rows), int(nw)) - 1.0


def meas_noise_table(m, v, amp=1.0):
    """The measurement-noise table of ClosedLoopMPC.set_meas_noise from a unit sample v (..., T, nw): amp v E[0]^T, the error in state coordinates.
    At amp = 1 this is exactly the set the tubes' stage-0 column assumes for the initial condition (Phi_x[0,0] = E[0])."""
    E = np.asarray(m.E, dtype=float)
    E0 = E[0] if E.ndim == 3 else E
    return float(amp) * (np.asarray(v, dtype=float) @ E0.T)


def can_run_persistent(rti, rti_steps, opts=None, environ=os.environ, sls_converge=False):
    """Whether ClosedLoopMPC.run_decoupled takes this setting (slsqp_cl_run / slsqp_cl_run_scp): any number of SCP iterations `rti` (<= 0: SCP
    converge mode), a fixed number of fast-SLS steps `rti_steps` >= 1 (None / <= 0 is fast-SLS converge mode: inside the loop only with
    sls_converge=True, run_decoupled's persistent_converge, and then with opts.max_sls_iter >= 1), fp64, and the fused chain with the shared first
    sweep allowed (opts.fuse_rti, SLSQP_FUSE_RTI, SLSQP_SWEEP_SHARED).  `opts`: a _lib.Opts (or anything with precision / fuse_rti attributes),
    None = the library's defaults.  Plain Python: needs no handle and no GPU."""
    if rti_steps is None or int(rti_steps) < 1:
        if not sls_converge or (opts is not None and int(getattr(opts, "max_sls_iter", 30)) < 1):
            return False
    if opts is not None and (int(getattr(opts, "precision", 0)) != 0 or int(getattr(opts, "fuse_rti", 1)) == 0):
        return False
    if opts is None and int(environ.get("SLSQP_PRECISION", "0") or 0) != 0:      # (BatchedFastSLS takes its precision from there)
        return False

    def env_on(name):
        v = environ.get(name)
        if v is None:
            return True
        try:
            return int(v) != 0
        except ValueError:
            return False      # (the library reads it with atoi: 0)
    return env_on("SLSQP_FUSE_RTI") and env_on("SLSQP_SWEEP_SHARED")


# rti = 1 with one fast-SLS step (the rocket script) takes the persistent launch by default, as before.  Plants whose script setting goes through
# slsqp_cl_run_scp take it by default only where it was measured faster (profiles/r04/README.md); for the others it is an option (persistent=True)
PERSISTENT_DEFAULT = {"pendulum": False, "quadrotor": False}


def _run_slice(model, N, seeds, steps, x0, device, noise, solve_nominal, continuation=1, budget_ms=None, persistent=None, x0_box_tol=0.0, solve_waves=1,
               reference=None, plant_params=None, bounds=None, solve_every=1, hold_trigger=None, plan_fallback=False, persistent_converge=False,
               adversary=None, adversary_amp=1.0, adversary_mask=None, meas_noise=None):
    B = len(seeds)
    W = np.stack([disturbance_stream(s, steps, model.nx) for s in seeds], axis=1) if noise else None   # (steps, B, nx)
    cl = ClosedLoopMPC(model, N, B, device=device, x0_box_tol=x0_box_tol, solve_waves=solve_waves, reference=reference, plant_params=plant_params, bounds=bounds, solve_every=solve_every, hold_trigger=hold_trigger, plan_fallback=plan_fallback,
                       adversary=adversary, adversary_amp=adversary_amp, adversary_mask=adversary_mask,
                       meas_noise=None if meas_noise is None else meas_noise_table(model, np.stack([measurement_stream(s, steps + 1, model.nw) for s in seeds]), meas_noise))
    X0 = np.tile(np.asarray(x0, dtype=float), (B, 1))
    rti_steps = cl.f.opts.rti_steps if cl.f.opts.rti_steps > 0 else None
    want = ((cl.rti == 1 and rti_steps == 1) or PERSISTENT_DEFAULT.get(getattr(model, "name", None), False)) if persistent is None else bool(persistent)
    # solve_every > 1 inside the persistent launch: only when asked for (persistent=True), for rti = 1 with one fast-SLS step and the persistent variant
    hold = solve_every > 1 and persistent is True and cl.rti == 1 and rti_steps == 1 and bool(cl.f.opts.cl_persistent) and solve_waves == 1
    if cl.hold_trigger < float("inf") and not hold:
        cl.close()
        raise ValueError("run_monte_carlo: hold_trigger runs in the persistent launch only: pass solve_every = M > 1 and persistent=True (rti = 1 with one fast-SLS step, opts.cl_persistent, solve_waves = 1)")
    # fast-SLS converge mode inside the persistent launch: only when asked for twice (persistent=True and persistent_converge=True)
    conv = bool(persistent_converge) and persistent is True and rti_steps is None and solve_every == 1 and solve_waves == 1
    if (solve_every == 1 or hold) and budget_ms != 0 and want and can_run_persistent(cl.rti, rti_steps, cl.f.opts, sls_converge=conv):      # instances advance independently (slsqp_cl_run / slsqp_cl_run_scp): same bits
        out = cl.run_decoupled(X0, steps, W, solve_nominal=solve_nominal, continuation=continuation, budget_ms=8.0 if budget_ms is None else budget_ms, persistent_hold=hold, persistent_converge=conv)
    else:
        out = cl.run_on_device(X0, steps, W, solve_nominal=solve_nominal, continuation=continuation)
    if cl.nlp_status is not None:
        out.update(nlp_status=cl.nlp_status, nlp_iterations=cl.nlp_iterations)
    cl.close()
    return out


def run_monte_carlo(model, N, seeds, steps, x0, rank=0, world=1, device=0, noise=True, gather=True, solve_nominal=False, slices=1, continuation=1,
                    budget_ms=None, persistent=None, x0_box_tol=0.0, solve_waves=1, reference=None, plant_params=None, bounds=None,
                    solve_every=1, hold_trigger=None, plan_fallback=False, persistent_converge=False,
                    adversary=None, adversary_amp=1.0, adversary_mask=None, meas_noise=None):
    """The rocket script's setting (rti = 1, one fast-SLS step) runs every slice's loop through slsqp_cl_run -- by default ONE persistent launch per slice in
    which no instance waits for another (budget_ms only matters for the round-based variant, ClosedLoopMPC.f.opts.cl_persistent = 0); budget_ms = 0 runs
    one slsqp_cl_step per step for the whole slice instead.  The results are the same bit for bit either way.
    persistent: None = the plant's default (PERSISTENT_DEFAULT), True = the persistent launch for every setting can_run_persistent accepts (the
    pendulum and quadrotor scripts' rti = 3 with 2 fast-SLS steps through slsqp_cl_run_scp), False = never.
    x0_box_tol: tolerance of the measured state against its own stage-0 box, for every slice and shard alike (ClosedLoopMPC; 0 = strict); the result
    holds `x0_violation` (seeds, steps, 2), the largest such violation of each step's first / last QP, whatever the tolerance.
    solve_waves: waves per instance of the QP solves (ClosedLoopMPC; above 1 the loops run step by step: for a handful of seeds).
    reference: what every seed tracks (ClosedLoopMPC.set_reference: "neutral", Xref or (Xref, Uref)); arrays with a leading axis of len(seeds)
    ((S,T,nx), (S,T,nu)) are per seed and are cut with the seeds into shards and slices.
    plant_params: the true plant of every seed (ClosedLoopMPC.set_plant_params: a dict, an array (np,), or per seed: an array (S,np) or a dict with
    (S,) entries, S = len(seeds)); what is per seed is cut with the seeds into shards and slices, exactly as a per-seed reference.  The result then
    holds `model_error` (seeds, nx, steps), `disturbance_used` (steps, seeds) and `plant_params` as given.
    bounds: the box of every seed over MPC time (ClosedLoopMPC.set_bounds: g or (g, gf)); arrays with a leading axis of len(seeds) ((S,T,ni),
    (S,T,ni_f)) are per seed and are cut with the seeds into shards and slices, as a per-seed reference is.  The result then holds
    `constraint_margin` (steps, seeds) and `bounds_g` / `bounds_gf` as given.
    solve_every: M > 1 = every seed's controller solves at steps 0, M, 2M, ... and holds its plan in between, the tube policy of the last solve acting on
    the measured state (ClosedLoopMPC.hold_step; 1 <= M <= N); the loops then run step by step and the result holds `hold_index` and `hold_policy`
    (seeds, steps).  With persistent=True, where can_run_persistent and the setting allow (rti = 1 with one fast-SLS step, opts.cl_persistent), the
    hold steps run inside the persistent launch instead (run_decoupled's persistent_hold): the same bits, plus `qp_stats`, `rounds`, `loop_stats`;
    persistent=None keeps stepping.  1 (default): today's loops, unchanged.
    hold_trigger: theta < inf = event-triggered solves (ClosedLoopMPC.run_decoupled's hold_trigger): with solve_every = M > 1 and persistent=True a seed's
    controller holds while its state stays inside theta x its tube and solves when it does not, or after M steps at the latest; the result then holds
    `tube_ratio` and `solve_trigger` (seeds, steps).  Without persistent=True it raises.  None (default): off.
    plan_fallback: True = a step of a seed that applies no freshly certified plan (a solve that failed, a hold step) runs the tube policy of the seed's
    last plan that succeeded (ClosedLoopMPC's plan_fallback; rti = 1 with one fast-SLS step); the result then holds `plan_age`, `hold_index` and
    `hold_policy` (seeds, steps), the policy as its code 0 / 1 / 2.  False (default): today's loops, unchanged.
    persistent_converge: True with persistent=True = a model in fast-SLS converge mode (model.fast_sls_rti_steps None, fast_SLS.solve's default) runs
    every slice as one persistent launch in which each seed iterates its solves to convergence on its own (run_decoupled's persistent_converge): the
    bits of the step-by-step loop, plus `qp_stats`, `rounds`, `loop_stats` and `sls_iterations` (seeds, steps).  persistent=None keeps stepping for
    this mode whatever the flag says.  False (default): today's loops, unchanged.
    adversary: "nearest_bound" / "away_from_target" = every seed's disturbance is decided on the device from its measured state
    (ClosedLoopMPC's adversary, adversary_amp, adversary_mask: the same for every seed); the seed's own stream stays the sample of the channels outside
    the mask.  The result then holds `w_applied` (steps, seeds, nx) and `disturbance_used` (steps, seeds), computed from it.  None / "off" (default):
    today's loops, unchanged.
    meas_noise: amp = every seed's controller is given x_meas = x_plant + amp E[0] v_s, v its own measurement_stream (steps + 1 rows), through
    ClosedLoopMPC's meas_noise (meas_noise_table); amp = 1 is the set the stage-0 column of the tubes assumes.  The result's `state_trajectory` then is
    the true trajectory, `measured_trajectory` what the controllers saw, `meas_noise` (seeds, steps + 1, nx) the tables.  None (default): today's loops,
    unchanged.
    slices > 1: the rank's seeds are cut into that many independent slices, each with its own handle (HIP stream) and host thread
    (as in fast_sls.SlicedDeviceBatch): results are bit-identical, the slices' solver tails overlap each other's bulk launches."""
    import threading
    seeds = np.asarray(seeds)
    S = len(seeds)
    lo, hi = shard_range(S, rank, world)
    mine = seeds[lo:hi]
    B = len(mine)
    K = max(1, min(int(slices), B))

    cuts = [(B * k // K, B * (k + 1) // K) for k in range(K)]

    def cut(k, v):
        """Rows [lo + a, lo + b) of a per-seed array (leading axis of len(seeds)) for slice k, the seeds [a, b) of this rank's shard; None stays None."""
        return None if v is None else np.asarray(v)[lo + cuts[k][0]:lo + cuts[k][1]]

    def per_seed(v, what):      # the length check of an option's first per-seed array (the arrays that follow it are cut as it is)
        if len(v) != S:
            raise ValueError(f"run_monte_carlo: {what} {S} leading rows, got {len(v)}")
        return v

    def options(k):      # reference, plant_params and bounds of slice k: what is per seed cut with the seeds, everything else as given
        kw = {}
        if reference is not None:
            Xr, Ur = reference if isinstance(reference, tuple) else (reference, None)
            kw["reference"] = (cut(k, per_seed(Xr, "a per-seed reference needs")), cut(k, Ur)) if np.ndim(Xr) == 3 else reference
        if isinstance(plant_params, dict):      # an entry is per seed from one axis on
            kw["plant_params"] = {}
            for name, v in plant_params.items():
                v = np.asarray(v, dtype=float)
                if v.ndim >= 1 and len(v) != S:
                    raise ValueError(f"run_monte_carlo: per-seed plant parameters need {S} leading rows, got {len(v)} ({name})")
                kw["plant_params"][name] = cut(k, v) if v.ndim >= 1 else v
        elif plant_params is not None:          # a bare array from two
            v = np.asarray(plant_params, dtype=float)
            kw["plant_params"] = cut(k, per_seed(v, "per-seed plant parameters need")) if v.ndim >= 2 else v
        if bounds is not None:
            gb, gfb = bounds if isinstance(bounds, (tuple, list)) and len(bounds) == 2 and np.ndim(bounds[0]) >= 2 else (bounds, None)
            kw["bounds"] = (cut(k, per_seed(gb, "per-seed bounds need")), cut(k, gfb)) if np.ndim(gb) == 3 else bounds
        return kw
    parts, err = [None] * K, []

    def work(k):
        try:
            kw = {} if persistent is None else dict(persistent=persistent)
            if x0_box_tol != 0.0:
                kw["x0_box_tol"] = x0_box_tol
            if solve_waves != 1:
                kw["solve_waves"] = solve_waves
            if solve_every != 1:
                kw["solve_every"] = solve_every
            if hold_trigger is not None:
                kw["hold_trigger"] = hold_trigger
            if plan_fallback:
                kw["plan_fallback"] = True
            if persistent_converge:
                kw["persistent_converge"] = True
            if adversary not in (None, "off", 0):
                kw.update(adversary=adversary, adversary_amp=adversary_amp, adversary_mask=adversary_mask)
            if meas_noise is not None:
                kw["meas_noise"] = float(meas_noise)
            kw.update(options(k))
            parts[k] = _run_slice(model, N, mine[cuts[k][0]:cuts[k][1]], steps, x0, device, noise, solve_nominal, continuation, budget_ms, **kw)
        except Exception as e:
            err.append(e)

    if K == 1:
        work(0)
    else:
        th = [threading.Thread(target=work, args=(k,)) for k in range(K)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    if err:
        raise err[0]
    out = {}
    for key, v in parts[0].items():
        if key in ("rounds", "loop_stats"):
            out[key] = [p[key] for p in parts]
        elif key in ("disturbance_used", "constraint_margin", "w_applied"):      # (steps, seeds[, nx])
            out[key] = np.concatenate([p[key] for p in parts], axis=1)
        elif key == "plant_params":      # as given: one vector, or a row per seed
            out[key] = v if v.ndim == 1 else np.concatenate([p[key] for p in parts], axis=0)
        elif key in ("bounds_g", "bounds_gf"):      # as given: shared rows, or a set per seed
            out[key] = v if v.ndim == 2 else np.concatenate([p[key] for p in parts], axis=0)
        elif isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == cuts[0][1] - cuts[0][0] and key not in ("t_jac", "t_qp", "t_riccati"):
            out[key] = np.concatenate([p[key] for p in parts], axis=0)
        elif key in ("t_qp", "t_riccati", "t_jac"):
            out[key] = np.max(np.stack([p[key] for p in parts]), axis=0)      # slices run concurrently
        else:
            out[key] = v
    res = dict(seeds=mine, **out)
    if gather and world > 1:
        import torch
        dev = torch.device("cuda", device) if torch.cuda.is_available() else torch.device("cpu")
        for k in ("state_trajectory", "input_trajectory"):
            t = torch.from_numpy(np.ascontiguousarray(out[k].reshape(B, -1))).to(dev)
            full = gather_rows(t, S, world).cpu().numpy()
            res[k + "_all"] = full.reshape((S,) + out[k].shape[1:])
    return res

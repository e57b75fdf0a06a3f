"""The closed-loop runs of tests/test_gpu_loop_args.py at their smallest shapes, as functions the test imports and as a program: run with
SLSQP_FUSE_RTI=0 in a process of its own (the switch is read once per process) it writes the step-by-step loop of every plant through the SEPARATE
launches -- k_qp_solve twice per step, its arguments from two independent make_qp_args calls -- to the .npz given on the command line."""
import os
import sys

import numpy as np

LOG_KEYS = ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x", "backoff_trajectory_u", "success",
            "scp_iterations", "primal_infeasibility", "x0_violation", "qp_stats")
FIN_KEYS = ("x_meas", "nominal_x", "nominal_u", "primal_vec")
# plant: (N, B, steps)
SHAPES = {"pendulum": (3, 5, 3), "quadrotor": (8, 5, 3), "rocket": (5, 5, 4)}
WAVES = 2      # SLSQP_LOOP_WAVES: fewer waves than instances, so every instance changes hands


def setup(name, N=None, B=None, steps=None):
    from robust_nonlinear_mpc_amd import disturbance_stream, get_model
    m = get_model(name)
    n, b, s = SHAPES[name]
    N, B, steps = N or n, B or b, steps or s
    if name == "rocket":
        x0, kw = np.tile(m.x_ref + 0.3 * (m.extra["x0"] - m.x_ref), (B, 1)), dict(solve_nominal=True, continuation=2)
    elif name == "quadrotor":
        x0, kw = np.tile(m.x_ref + 0.02 * (m.x_ub - m.x_lb), (B, 1)), dict(solve_nominal=True)
    else:
        x0, kw = np.tile(m.extra["x0"], (B, 1)), dict(solve_nominal=True)
    x0 = x0 * (1.0 + 0.05 * np.arange(B)[:, None] / B) if name != "quadrotor" else x0      # (instances differ; the quaternion stays a unit one)
    W = np.stack([disturbance_stream(s_, steps, m.nx) for s_ in range(B)], axis=1)
    return m, N, B, steps, x0, W, kw


def make(m, N, B, tune=None, rti=1, rti_steps=1, reference=None, plant_params=None, bounds=None):
    from robust_nonlinear_mpc_amd import ClosedLoopMPC
    cl = ClosedLoopMPC(m, N, B, rti=rti, fast_sls_rti_steps=rti_steps, reference=reference, plant_params=plant_params, bounds=bounds)
    if tune:
        tune(cl.f.opts)
    return cl


def final(cl):
    m, N = cl.m, cl.N
    return {k: cl.f.get(k, shp) for k, shp in (("x_meas", (m.nx,)), ("nominal_x", (N + 1, m.nx)), ("nominal_u", (N, m.nu)), ("primal_vec", (cl.f.n,)))}


def stepwise(cl, steps, x0, W, close=True, **kw):
    """One slsqp_cl_step per MPC step with the device-side log on, qp_stats read after each."""
    L = __import__("robust_nonlinear_mpc_amd")._lib
    L.check(cl.f.lib.slsqp_cl_log(cl.f.h, steps))
    cl.reset(x0, **kw)
    stats = []
    for i in range(steps):
        cl.step(W[i], fetch=False)
        stats.append(cl.f.get("qp_stats", (2, 8), np.int32))
    out = cl._log_result(steps, np.zeros((steps, 1)), np.zeros((steps, 1)), np.zeros((steps, 1)))
    out["qp_stats"] = np.stack(stats, axis=1)
    fin = final(cl)
    if close:
        cl.close()
    return out, fin


def decoupled(cl, steps, x0, W, close=True, **kw):
    """slsqp_cl_run / slsqp_cl_run_scp with WAVES waves."""
    os.environ["SLSQP_LOOP_WAVES"] = str(WAVES)
    try:
        out = cl.run_decoupled(x0, steps, W, **kw)
    finally:
        os.environ.pop("SLSQP_LOOP_WAVES", None)
    fin = final(cl)
    if close:
        cl.close()
    return out, fin


def real_work(out):
    """Both statistics slots filled by QPs that ran block solves, in every step."""
    q = out["qp_stats"]      # (B, steps, 2, 8)
    return bool(((q[:, :, :, 6] != -1) & (q[:, :, :, 1] > 0)).any(axis=0).all())


def assert_same(out, fin, ref, ref_fin, what=""):
    for k in LOG_KEYS:
        assert np.array_equal(out[k], ref[k], equal_nan=True), (what, k)
    for k in FIN_KEYS:
        assert np.array_equal(fin[k], ref_fin[k], equal_nan=True), (what, k)


# ---- the per-handle options: every state (reference, plant parameters, bounds) on or off, tests/test_gpu_option_states.py and scripts/option_state_bits.py
STATES = [(r, p, b) for r in (0, 1) for p in (0, 1) for b in (0, 1)]


def option_state(m, B, state, T=2):
    """make()'s keywords for one state: per-instance tables of T rows (shorter than steps + N: the held last row is in every window), the box with an
    input limit of 0.22 and every side pulled in by up to 10 %, the reference up to 0.1 off the neutral point, the parameters up to 10 % off their
    defaults; all differ per instance and row."""
    from robust_nonlinear_mpc_amd._plant_cli import sample_plant_params
    ref, pp, bnd = state
    t, b = np.arange(T)[None, :, None], np.arange(B)[:, None, None]
    kw = {}
    if ref:
        Xref = np.tile(np.asarray(m.x_ref, dtype=float), (B, T, 1))
        Xref[:, :, :1] += 0.1 * np.sin(0.35 * t + 0.7 * b + 1.0)
        kw["reference"] = (Xref, np.tile(np.asarray(m.u_ref, dtype=float), (B, T, 1)))
    if pp:
        kw["plant_params"] = sample_plant_params(m, 1000 + np.arange(B), 10.0)
    if bnd:
        def pull(base):
            return np.asarray(base, dtype=float) * (1.0 - 0.1 * (0.5 + 0.5 * np.sin(0.35 * t + 0.7 * b + 0.3 * np.arange(len(base))[None, None, :])))
        g = np.array(m.g, dtype=float)
        g[m.nx:m.nz] = g[m.nz + m.nx:] = 0.22      # (the pendulum's first inputs are -0.24 without it: the rows are active)
        kw["bounds"] = (pull(g), pull(m.gf))
    return kw


def _tune(**fields):
    def tune(o):
        for k, v in fields.items():
            setattr(o, k, v)
    return tune


def option_state_runs(state, name="pendulum"):
    """Every closed-loop route of one state at the plant's smallest shape: {route: (out, fin)}.  step0 / step2: one slsqp_cl_step per step through the
    separate launches / the fused chain; persistent, rounds: slsqp_cl_run; scp_step, scp: rti = 2 with two fast-SLS steps, step by step and
    slsqp_cl_run_scp.  Every run starts with slsqp_nominal_solve."""
    m, N, B, steps, x0, W, kw = setup(name)
    mk = option_state(m, B, state)
    scp = dict(rti=2, rti_steps=2, **mk)
    return {"step0": stepwise(make(m, N, B, _tune(fuse_rti=0), **mk), steps, x0, W, **kw),
            "step2": stepwise(make(m, N, B, _tune(fuse_rti=2), **mk), steps, x0, W, **kw),
            "persistent": decoupled(make(m, N, B, **mk), steps, x0, W, **kw),
            "rounds": decoupled(make(m, N, B, _tune(cl_persistent=0), **mk), steps, x0, W, **kw),
            "scp_step": stepwise(make(m, N, B, **scp), steps, x0, W, **kw),
            "scp": decoupled(make(m, N, B, **scp), steps, x0, W, **kw)}


def main(path):
    assert os.environ.get("SLSQP_FUSE_RTI") == "0"
    arrays = {}
    for name in SHAPES:
        m, N, B, steps, x0, W, kw = setup(name)
        out, fin = stepwise(make(m, N, B), steps, x0, W, **kw)
        for k in LOG_KEYS:
            arrays[f"{name}/{k}"] = out[k]
        for k in FIN_KEYS:
            arrays[f"{name}/fin/{k}"] = fin[k]
    np.savez(path, **arrays)
    print("loop_args_runs ok")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main(sys.argv[1])

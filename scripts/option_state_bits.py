"""Every closed-loop route in every state of the per-handle options (reference, plant parameters, bounds on or off) at the smallest shape, all logs
and final arrays into ONE .npz: run once per library (SLSQP_SO names another build) and compare the two files, which must be identical bit for bit
when a change claims to leave the arithmetic alone.

    python scripts/option_state_bits.py OUT.npz            # the runs of tests/loop_args_runs.py::option_state_runs, pendulum N = 3, B = 5, 3 steps
    python scripts/option_state_bits.py A.npz B.npz        # compare: prints every array that differs, exit status 1 if any does

A second group, "solve/...", holds the solve-level routes the closed loops do not take (solve_routes below): slsqp_solve through the separate
launches, the fused chain, two fast-SLS steps, converge mode, mixed precision, two waves per instance and a non-zero x0 tolerance on both routes,
each called twice (a handle's first and second solve); slsqp_qp_solve cold then warm; slsqp_sweep with the box and with a general G; and a
step-by-step closed loop in which one instance fails its first SCP iteration, so that the second solve of every step runs with a mask that leaves
it out.  Pendulum N = 3 and quadrotor N = 8, B = 5.

    SLSQP_SO=<a library built with -DSLSQP_EXTRA_DIMS="X(6,2)"> python scripts/option_state_bits.py --extra-dims OUT.npz
                                                            # tests/dims_extra_check.py as test_extra_dims_build runs it, its result arrays
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _state(f):
    """What a solve-level run leaves in the handle: test_gpu_sweep_routes.fetch (primal, dual, status, eta, K, beta, back-offs, ...), the QP
    iteration counts, qp_stats and the x0 record."""
    from test_gpu_sweep_routes import fetch
    r = fetch(f)
    r["qp_iters"], r["qp_stats"], r["x0_viol"] = f.get("qp_iters", (), np.int32), f.get("qp_stats", (2, 8), np.int32), f.get("x0_viol", (2,))
    return r


def solve_routes():
    """{route: {array name: array}} of the second group."""
    import loop_args_runs as R
    from problems import make_gpu_solver, push_instances, stack
    from robust_nonlinear_mpc_amd import BatchedFastSLS, get_model
    from sweep_cases import make_case
    from conftest import GOLDEN
    routes = {"separate": dict(fuse_rti=0), "fused": dict(fuse_rti=2), "rti2": dict(rti_steps=2, fuse_rti=0, conv_tol=-1.0), "converge": dict(rti_steps=0),
              "precision1": dict(precision=1), "waves2": dict(solve_waves=2), "x0tol_separate": dict(fuse_rti=0, x0_box_tol=1e-2),
              "x0tol_fused": dict(fuse_rti=2, x0_box_tol=1e-2)}
    out = {}
    for model, N in (("pendulum", 3), ("quadrotor", 8)):
        insts = make_case(model, N, "model", 5)
        x0 = stack(insts, "x0_arg")
        x0_out = x0.copy()      # instance 0 pinned 5e-3 outside its stage-0 box: refused by the strict gate, accepted with the tolerance 1e-2
        x0_out[0, 0] = -(insts[0].g_list[0][0] + 5e-3)
        for route, o in routes.items():
            f = make_gpu_solver(insts)
            f.set_rti_steps(o.get("rti_steps", 1))
            for k, v in o.items():
                if k != "rti_steps":
                    setattr(f.opts, k, v)
            for call in (1, 2):      # the handle's first solve, then one that begins with k_solve_begin
                push_instances(f, insts)
                f.solve(x0_out if route in ("separate", "fused") or "x0tol" in route else x0, fetch=False)
                out[f"{model}/{route}/call{call}"] = _state(f)
            f.close()
        f = make_gpu_solver(insts)      # slsqp_qp_solve on the handle's QP (x_0 pinned to 0), cold then warm
        push_instances(f, insts)
        for warm in (0, 1):
            f.opts.warm_start = warm
            x, y, st, it, _ = f.qp_solve()
            out[f"{model}/qp_solve/warm{warm}"] = dict(x=x, y=y, status=st, iters=it, qp_stats=f.get("qp_stats", (2, 8), np.int32))
        eta, eta_f = out[f"{model}/separate/call1"]["eta"], out[f"{model}/separate/call1"]["eta_f"]
        out[f"{model}/sweep_box"] = f.sweep(eta, eta_f)      # slsqp_sweep, G = [I; -I], on the eta of the first route
        f.close()
        if model == "pendulum":      # one instance starts outside its state box: its steps fail, and the second SCP iteration's solve leaves it out
            m, N_, B, steps, xm, W, kw = R.setup(model)
            xm = xm.copy()
            xm[4] = m.x_ub + 0.1 * (m.x_ub - m.x_lb)
            log, fin = R.stepwise(R.make(m, N_, B, rti=2), steps, xm, W, **kw)
            assert not log["success"][4].any() and log["success"][:4].any(), log["success"]
            out[f"{model}/masked_steps"] = {**{k: log[k] for k in R.LOG_KEYS}, **{"fin/" + k: fin[k] for k in R.FIN_KEYS}}
    g = dict(np.load(os.path.join(GOLDEN, "sweep_pendulum_N10_s1_genG.npz")))      # slsqp_sweep with a general G (tests/test_gpu_parity.py)
    from types import SimpleNamespace
    base, N, B = get_model("pendulum"), int(g["N"]), 3
    m = SimpleNamespace(nx=base.nx, nu=base.nu, nw=base.nw, ni=int(g["ni"]), ni_f=int(g["ni_f"]), G=g["G"], Gf=g["Gf"], gf=np.zeros(int(g["ni_f"])), E=base.E,
                        Q=base.Q, R=base.R, Qf=base.Qf)
    f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, g["Q_reg"], g["R_reg"], g["Q_reg_f"], batch=B)
    A = np.stack([g["A"] * (1.0 + 1e-2 * b) for b in range(B)])
    f.update_dynamics_list(A, np.stack([g["B"]] * B), g["E"], np.zeros((B, N, m.ni)), np.zeros((B, m.ni_f)), np.zeros((B, N, m.nx)))
    out["pendulum/sweep_general_G"] = f.sweep(np.stack([g["eta"]] * B), np.stack([g["eta_f"]] * B))
    f.close()
    return out


def record_extra_dims(path):
    import runpy
    from robust_nonlinear_mpc_amd import _lib
    res = runpy.run_path(os.path.join(ROOT, "tests", "dims_extra_check.py"))["out"]      # (its own assertions run)
    arrays = {f"dims62/{k}": v for k, v in res.items() if isinstance(v, np.ndarray)}
    np.savez(path, **arrays)
    print("option_state_bits:", len(arrays), "arrays from", _lib.SO_PATH, "->", path)


def record(path):
    import loop_args_runs as R
    from robust_nonlinear_mpc_amd import _lib
    arrays = {f"solve/{route}/{k}": v for route, r in solve_routes().items() for k, v in r.items()}
    print("option_state_bits:", len(arrays), "arrays of the solve-level routes")
    for state in R.STATES:
        tag = "".join(map(str, state))
        m, N, B, steps, x0, W, kw = R.setup("pendulum")
        cl = R.make(m, N, B, **R.option_state(m, B, state))      # slsqp_nominal_solve alone
        cl.reset(x0, **kw)
        for k, v in R.final(cl).items():
            arrays[f"{tag}/nominal_solve/{k}"] = v
        cl.close()
        for route, (out, fin) in R.option_state_runs(state).items():
            assert R.real_work(out), (tag, route)
            for k in R.LOG_KEYS:
                arrays[f"{tag}/{route}/{k}"] = out[k]
            for k in R.FIN_KEYS:
                arrays[f"{tag}/{route}/fin/{k}"] = fin[k]
    np.savez(path, **arrays)
    print("option_state_bits:", len(arrays), "arrays from", _lib.SO_PATH, "->", path)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files)) + [k for k in A.files if k in B.files and not np.array_equal(A[k], B[k], equal_nan=True)]
    for k in bad:
        print("differs:", k)
    print("option_state_bits:", len(A.files), "arrays,", len(bad), "differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--extra-dims":
        sys.exit(record_extra_dims(sys.argv[2]))
    sys.exit(compare(*sys.argv[1:3]) if len(sys.argv) > 2 else record(sys.argv[1]))

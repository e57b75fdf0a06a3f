"""The persistent closed-loop launch for multi-iteration SCP and multi-step fast-SLS (slsqp_cl_run_scp, k_cl_loop_scp) against one slsqp_cl_step per
MPC step on a fresh handle: per instance the same operations in the same order, so every logged array, every per-QP statistic and the final state
are identical bit for bit -- for the pendulum / quadrotor script settings (rti = 3, two fast-SLS steps), other (rti, rti_steps) pairs, SCP converge
mode (every instance leaves the loop at its own iteration), with fewer waves than instances, and with an instance that fails.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOG_KEYS = ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x", "backoff_trajectory_u", "success",
            "scp_iterations", "primal_infeasibility")


def _final(cl):
    m, N = cl.m, cl.N
    return {k: cl.f.get(k, shp) for k, shp in (("x_meas", (m.nx,)), ("nominal_x", (N + 1, m.nx)), ("nominal_u", (N, m.nu)), ("primal_vec", (cl.f.n,)))}


def _make(m, N, B, rti, rti_steps, tune=None, setup=None):
    """tune(opts) adjusts the handle's options, setup(cl) anything else on the freshly constructed loop (tests/test_gpu_sweep_routes.py: its E)."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC
    cl = ClosedLoopMPC(m, N, B, rti=rti, fast_sls_rti_steps=rti_steps)
    if tune:
        tune(cl.f.opts)
    if setup:
        setup(cl)
    return cl


def _stepwise(m, N, B, steps, x0, W, rti, rti_steps, tune=None, setup=None, inspect=None, **reset_kw):
    """The reference side: one slsqp_cl_step per MPC step, qp_stats read after each.  inspect(cl) sees the loop after its last step, before it is closed."""
    L = __import__("robust_nonlinear_mpc_amd")._lib
    cl = _make(m, N, B, rti, rti_steps, tune, setup)
    assert L.load().slsqp_cl_log(cl.f.h, steps) == 0
    cl.reset(x0, **reset_kw)
    stats = []
    for i in range(steps):
        cl.step(None if W is None else W[i], fetch=False)
        stats.append(cl.f.get("qp_stats", (2, 8), np.int32))
    ref = cl._log_result(steps, np.zeros((steps, 1)), np.zeros((steps, 1)), np.zeros((steps, 1)))
    ref["qp_stats"] = np.stack(stats, axis=1)
    fin = _final(cl)
    if inspect:
        inspect(cl)
    cl.close()
    return ref, fin


def _persistent(m, N, B, steps, x0, W, rti, rti_steps, tune=None, waves=None, setup=None, **reset_kw):
    cl = _make(m, N, B, rti, rti_steps, tune, setup)
    if waves is not None:
        os.environ["SLSQP_LOOP_WAVES"] = str(waves)
    try:
        out = cl.run_decoupled(x0, steps, W, **reset_kw)
    finally:
        os.environ.pop("SLSQP_LOOP_WAVES", None)
    fin = _final(cl)
    cl.close()
    return out, fin


def _assert_same(out, fin, ref, ref_fin, B, steps, waves=None):
    for k in LOG_KEYS:
        assert np.array_equal(out[k], ref[k], equal_nan=True), k
    assert np.array_equal(out["qp_stats"], ref["qp_stats"]), "qp_stats"
    for k in fin:
        assert np.array_equal(fin[k], ref_fin[k], equal_nan=True), k
    ls = out["loop_stats"]
    assert out["rounds"] == 1 and ls["mpc_steps"] == B * steps and ls["busy_ms"] > 0, ls
    assert ls["waves"] == (B if waves is None else waves), ls


def _seeded_W(m, B, steps):
    from robust_nonlinear_mpc_amd import disturbance_stream
    return np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)


def _script_x0(m, B):
    return np.tile(m.extra["x0"], (B, 1)) if "x0" in m.extra else np.tile(m.x_ref + 0.02 * (m.x_ub - m.x_lb), (B, 1))


@pytest.mark.parametrize("model,N,B,steps,waves", [("pendulum", 10, 200, 12, None), ("quadrotor", 20, 150, 8, None), ("quadrotor", 20, 150, 8, 30)])
def test_script_settings_of_pendulum_and_quadrotor_are_bitwise_the_step_by_step_loop(model, N, B, steps, waves):
    """rti = 3 with two fast-SLS steps per solve (models.py: the pendulum and quadrotor scripts' own values): three linearisations and nine QPs per MPC
    step, the second fast-SLS step through the general per-column sweep.  waves = 30 is the over-subscribed regime forced on a small batch: every
    wave serves five instances through the queue, instances change waves between their MPC steps."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    assert (m.rti, m.fast_sls_rti_steps) == (3, 2)
    x0, W = _script_x0(m, B), _seeded_W(m, B, steps)
    ref, ref_fin = _stepwise(m, N, B, steps, x0, W, None, None, solve_nominal=True)
    out, fin = _persistent(m, N, B, steps, x0, W, None, None, waves=waves, solve_nominal=True)
    _assert_same(out, fin, ref, ref_fin, B, steps, waves)
    if waves is not None:
        assert out["loop_stats"]["waves"] < B
    assert ref["success"].mean() > 0.5 and (ref["scp_iterations"][ref["success"]] == 2).all()      # (iterations are counted from 0)


@pytest.mark.parametrize("waves", [None, 7])
@pytest.mark.parametrize("rti,rti_steps", [(3, 2), (2, 1), (1, 3)])
def test_rocket_other_settings_are_bitwise_the_step_by_step_loop(rti, rti_steps, waves):
    """Rocket from the script's x0, 96 seeds x 10 steps: several SCP iterations with one fast-SLS step, one iteration with three (two general
    sweeps, two middle QPs), and both; with as many waves as instances and with 7 (instances change hands between waves)."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("rocket")
    N, B, steps = 20, 96, 10
    x0, W = np.tile(m.extra["x0"], (B, 1)), _seeded_W(m, B, steps)
    ref, ref_fin = _stepwise(m, N, B, steps, x0, W, rti, rti_steps, solve_nominal=True, continuation=2)
    out, fin = _persistent(m, N, B, steps, x0, W, rti, rti_steps, waves=waves, solve_nominal=True, continuation=2)
    _assert_same(out, fin, ref, ref_fin, B, steps, waves)
    assert ref["success"].mean() > 0.5


@pytest.mark.parametrize("model,N,steps,amp,scp_eps", [("pendulum", 10, 2, 0.04, 1e-8), ("rocket", 20, 1, 0.01, 1e-6)])
def test_scp_converge_mode_is_bitwise_the_step_by_step_loop(model, N, steps, amp, scp_eps):
    """rti = -1 with two fast-SLS steps (scp_eps / max_scp_iter as in test_closed_loop_scp_converge_mode_vs_oracle): inside the launch an instance
    leaves the SCP loop when ITS step is below scp_eps, where the step-by-step loop reads a batch-wide counter back after every iteration.  The
    initial states spread from the reference point to `amp` of the box, so the instances need different numbers of iterations."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    B = 12
    rng = np.random.default_rng(23)
    x0 = np.stack([m.x_ref + amp * (b / (B - 1)) * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, m.nx) for b in range(B)])

    def tune(o):
        o.scp_eps = scp_eps
    ref, ref_fin = _stepwise(m, N, B, steps, x0, None, -1, 2, tune)
    print("scp_iterations (step-by-step):", ref["scp_iterations"].tolist())
    assert len(set(ref["scp_iterations"][:, 0].tolist())) > 1      # instances really leave at different iterations
    out, fin = _persistent(m, N, B, steps, x0, None, -1, 2, tune)
    _assert_same(out, fin, ref, ref_fin, B, steps)
    assert ref["success"].any()


def test_failing_instance_is_masked_and_the_run_drains():
    """Instance 1 starts far outside its box (as in test_one_infeasible_instance_does_not_fail_the_batch): its first QP of every MPC step is
    infeasible, the step-by-step loop masks it for the remaining SCP iterations of the step (scp_active), and so does the launch; the other
    instances are untouched and the queue drains."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, steps = 10, 16, 5
    x0 = np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.2 * np.random.default_rng(3).uniform(-1, 1, (B, 1)))
    x0[1] += 100.0
    ref, ref_fin = _stepwise(m, N, B, steps, x0, None, 3, 2)
    out, fin = _persistent(m, N, B, steps, x0, None, 3, 2)
    _assert_same(out, fin, ref, ref_fin, B, steps)
    assert not out["success"][1].any() and (out["scp_iterations"][1] == 0).all()
    assert (out["qp_stats"][1, :, :, 6] == -1).all()          # its last SCP iteration of every step took no part in any QP
    others = np.arange(B) != 1
    assert out["success"][others].mean() > 0.5
    clean, _ = _persistent(m, N, B - 1, steps, x0[others], None, 3, 2)
    for k in LOG_KEYS:
        assert np.array_equal(out[k][others], clean[k], equal_nan=True), k


def test_one_iteration_one_step_through_the_new_entry_point_is_slsqp_cl_run():
    """rti = 1 with rti_steps = 1 through slsqp_cl_run_scp dispatches to slsqp_cl_run's own persistent kernel: same bits."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model
    L = __import__("robust_nonlinear_mpc_amd")._lib
    m = get_model("rocket")
    N, B, steps = 20, 64, 6
    x0, W = np.tile(m.extra["x0"], (B, 1)), _seeded_W(m, B, steps)
    cl = ClosedLoopMPC(m, N, B)
    ref = cl.run_decoupled(x0, steps, W, solve_nominal=True, continuation=2)
    ref_fin = _final(cl)
    cl.close()
    cl = ClosedLoopMPC(m, N, B)
    assert (cl.rti, cl.f.opts.rti_steps) == (1, 1)
    L.check(cl.f.lib.slsqp_cl_log(cl.f.h, steps))
    cl.reset(x0, solve_nominal=True, continuation=2)
    Wc = np.ascontiguousarray(W)
    L.check(cl.f.lib.slsqp_cl_run_scp(cl.f.h, steps, 1, Wc.ctypes.data_as(C.c_void_p), L.HOST, C.byref(cl.f.opts)))
    out = cl._log_result(steps, np.zeros((steps, 1)), np.zeros((steps, 1)), np.zeros((steps, 1)))
    out["qp_stats"] = cl.f.get("log_qp_stats", (steps, 2, 8), np.int32)
    fin = _final(cl)
    cl.close()
    for k in LOG_KEYS + ("qp_stats",):
        assert np.array_equal(out[k], ref[k], equal_nan=True), k
    for k in fin:
        assert np.array_equal(fin[k], ref_fin[k], equal_nan=True), k


@pytest.mark.parametrize("model,rti,rti_steps", [("rocket", None, None), ("pendulum", None, None)])
def test_two_runs_of_different_length_on_one_handle(model, rti, rti_steps):
    """10 and then 5 steps on one ClosedLoopMPC: log_qp_stats is registered and indexed with the current run's step count (its allocation only grows)."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    N, B = (20 if model == "rocket" else 10), 8
    cl = _make(m, N, B, rti, rti_steps)
    x0 = _script_x0(m, B)
    cont = 2 if model == "rocket" else 1          # (the script's rocket x0 is far from hover: the initialiser gets there in two stages, as in the other rocket tests)
    a = cl.run_decoupled(x0, 10, _seeded_W(m, B, 10), solve_nominal=True, continuation=cont)
    b = cl.run_decoupled(x0, 5, _seeded_W(m, B, 5), solve_nominal=True, continuation=cont)
    cl.close()
    assert a["qp_stats"].shape == (B, 10, 2, 8) and b["qp_stats"].shape == (B, 5, 2, 8)
    assert a["success"].any() and b["success"].any()
    assert (b["qp_stats"][:, :, 1, 1] > 0).any()          # every step of the short run has its own entries
    assert np.array_equal(a["state_trajectory"][:, :, 0], b["state_trajectory"][:, :, 0])


def test_unsupported_settings_are_refused_with_their_reason():
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model
    L = __import__("robust_nonlinear_mpc_amd")._lib
    m = get_model("pendulum")
    cl = ClosedLoopMPC(m, 10, 4)
    cl.reset(np.tile(m.extra["x0"], (4, 1)))
    lib = cl.f.lib
    cl.f.opts.rti_steps = 0
    assert lib.slsqp_cl_run_scp(cl.f.h, 2, 3, None, L.HOST, C.byref(cl.f.opts)) < 0
    assert "rti_steps" in lib.slsqp_last_error().decode()
    cl.f.opts.rti_steps = 2
    cl.f.opts.precision = 1
    assert lib.slsqp_cl_run_scp(cl.f.h, 2, 3, None, L.HOST, C.byref(cl.f.opts)) < 0
    assert "precision" in lib.slsqp_last_error().decode()
    cl.f.opts.precision = 0
    cl.f.set_rti_steps(None)
    with pytest.raises(RuntimeError, match="rti_steps"):
        cl.run_decoupled(np.tile(m.extra["x0"], (4, 1)), 2)
    cl.f.set_rti_steps(2)
    out = cl.run_decoupled(np.tile(m.extra["x0"], (4, 1)), 2)          # the handle is still usable
    cl.close()
    assert out["success"].any() and out["loop_stats"]["mpc_steps"] == 4 * 2


@pytest.mark.parametrize("model,N,steps,amp", [("pendulum", 10, 4, 1.0), ("quadrotor", 20, 3, 1.0)])
def test_persistent_scp_closed_loop_vs_oracle(model, N, steps, amp):
    """The persistent launch at the script settings against the CPU restatement of SCP_SLS.solve / reset_warm_start built on the oracle: initial
    states and tolerances of test_closed_loop_vs_oracle (tests/test_gpu_parity.py)."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model
    from problems import run_oracle_closed_loop
    m = get_model(model)
    B = 3
    rng = np.random.default_rng(11)
    x0 = np.stack([m.x_ref + amp * 0.05 * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, m.nx) for _ in range(B)])
    if model == "pendulum":
        x0[0] = m.extra["x0"]
    if model == "quadrotor":
        D = np.array([2.0] * 3 + [1.0] * 3 + [0.0] + [0.1] * 3 + [0.5] * 3)
        x0 = m.x_ref + D * rng.uniform(-1, 1, (B, m.nx))
        x0[:, 6:10] /= np.linalg.norm(x0[:, 6:10], axis=1, keepdims=True)
    cl = ClosedLoopMPC(m, N, B)
    out = cl.run_decoupled(x0, steps, None)
    cl.close()
    assert out["loop_stats"]["mpc_steps"] == B * steps
    for b in range(B):
        ref = run_oracle_closed_loop(m, N, x0[b], steps, m.rti, m.fast_sls_rti_steps, None)
        assert list(out["success"][b]) == list(ref["success"])
        scale = max(1.0, np.abs(ref["nominal_x"]).max())
        assert np.max(np.abs(out["state_trajectory"][b].T - ref["state"])) < 1e-6 * scale
        assert np.max(np.abs(out["input_trajectory"][b].T - ref["u0"][: steps - 1])) < 1e-6 * max(1.0, np.abs(ref["u0"]).max())
        assert np.max(np.abs(out["nominal_trajectory_x"][b].transpose(2, 1, 0) - ref["nominal_x"])) < 1e-6 * scale
        for i in range(steps):
            if ref["backoff_x"][i] is not None:
                assert np.allclose(out["backoff_trajectory_x"][b][:, :, i].T, ref["backoff_x"][i], rtol=1e-5, atol=1e-8)
        ok = np.array(ref["success"], dtype=bool)
        assert np.allclose(out["primal_infeasibility"][b][ok], np.array(ref["primal_infeasibility"])[ok], rtol=1e-4, atol=1e-9)

"""Fast-SLS converge mode inside the persistent closed-loop launch (slsqp_cl_set_sls_converge, the CONV variants of k_cl_loop_scp) against one
slsqp_cl_step per MPC step on a fresh handle: per instance the same operations in the same order, so every logged array, every per-QP statistic,
the stage-0 record, the iteration counts and the final state are identical bit for bit -- while inside the launch every instance leaves its
fast-SLS loop at its own iteration, where the step-by-step loop reads a batch-wide counter back after every iteration and goes on until its slowest
instance has left.  The helpers are those of tests/test_gpu_cl_scp.py.

Initial states: x0[b] = x_ref + amp (b / (B - 1)) (x_ub - x_lb) u_b, u_b uniform in [-1, 1]^nx from default_rng(23), B = 6, no noise: the
instances spread from the reference point outwards and need different numbers of iterations (each test asserts so on the step-by-step side)."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOG_KEYS = ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x", "backoff_trajectory_u", "success",
            "scp_iterations", "primal_infeasibility")
B6 = 6


def _final(cl):
    m, N = cl.m, cl.N
    return {k: cl.f.get(k, shp) for k, shp in (("x_meas", (m.nx,)), ("nominal_x", (N + 1, m.nx)), ("nominal_u", (N, m.nu)), ("primal_vec", (cl.f.n,)))}


def _make(m, N, B, rti, tune=None, setup=None):
    """Fast-SLS converge mode (fast_sls_rti_steps None with an explicit rti).  tune(opts) adjusts the handle's options, setup(cl) anything else."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC
    cl = ClosedLoopMPC(m, N, B, rti=rti, fast_sls_rti_steps=None)
    assert cl.f.opts.rti_steps == 0
    if tune:
        tune(cl.f.opts)
    if setup:
        setup(cl)
    return cl


def _stepwise(m, N, B, steps, x0, rti, tune=None, setup=None):
    """The reference side: one slsqp_cl_step per MPC step; qp_stats and iteration_number read after each."""
    L = __import__("robust_nonlinear_mpc_amd")._lib
    cl = _make(m, N, B, rti, tune, setup)
    assert L.load().slsqp_cl_log(cl.f.h, steps) == 0
    cl.reset(x0)
    stats, its = [], []
    for i in range(steps):
        cl.step(None, fetch=False)
        stats.append(cl.f.get("qp_stats", (2, 8), np.int32))
        its.append(cl.f.get("iteration_number", (), np.int32))
    ref = cl._log_result(steps, np.zeros((steps, 1)), np.zeros((steps, 1)), np.zeros((steps, 1)))
    ref["qp_stats"] = np.stack(stats, axis=1)
    ref["sls_iterations"] = np.stack(its, axis=1)
    fin = _final(cl)
    cl.close()
    return ref, fin


def _persistent(m, N, B, steps, x0, rti, tune=None, waves=None, setup=None):
    cl = _make(m, N, B, rti, tune, setup)
    if waves is not None:
        os.environ["SLSQP_LOOP_WAVES"] = str(waves)
    try:
        out = cl.run_decoupled(x0, steps, None, persistent_converge=True)
    finally:
        os.environ.pop("SLSQP_LOOP_WAVES", None)
    assert not cl.f.get_sls_converge()          # the option was this call's
    fin = _final(cl)
    cl.close()
    return out, fin


def _assert_same(out, fin, ref, ref_fin, B, steps, waves=None):
    for k in LOG_KEYS:
        assert np.array_equal(out[k], ref[k], equal_nan=True), k
    assert np.array_equal(out["qp_stats"], ref["qp_stats"]), "qp_stats"
    assert np.array_equal(out["x0_violation"], ref["x0_violation"], equal_nan=True), "x0_violation"
    assert out["sls_iterations"].dtype == np.int32 and out["sls_iterations"].shape == (B, steps)
    assert np.array_equal(out["sls_iterations"], ref["sls_iterations"]), "sls_iterations"
    for k in fin:
        assert np.array_equal(fin[k], ref_fin[k], equal_nan=True), k
    ls = out["loop_stats"]
    assert out["rounds"] == 1 and ls["mpc_steps"] == B * steps and ls["busy_ms"] > 0, ls
    assert ls["waves"] == (B if waves is None else waves), ls


def _spread_x0(m, amp, B=B6):
    rng = np.random.default_rng(23)
    return np.stack([m.x_ref + amp * (b / (B - 1)) * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, m.nx) for b in range(B)])


_cache = {}


def _quadrotor_case():
    """Case 1's two sides, computed once and left unchanged (the tests below share them)."""
    if "quad" not in _cache:
        from robust_nonlinear_mpc_amd import get_model
        m = get_model("quadrotor")
        x0 = _spread_x0(m, 0.05)
        _cache["quad"] = (m, x0, _stepwise(m, 4, B6, 2, x0, 2), _persistent(m, 4, B6, 2, x0, 2))
    return _cache["quad"]


def test_quadrotor_every_instance_at_its_own_iteration_is_bitwise_the_step_by_step_loop():
    """Quadrotor, N = 4, rti = 2, 2 steps: on the CPU oracle the instances need 1, 1, 1, 1, 3, 4 iterations per solve."""
    m, x0, (ref, ref_fin), (out, fin) = _quadrotor_case()
    print("sls_iterations (step-by-step):", ref["sls_iterations"].tolist())
    assert len(set(ref["sls_iterations"][:, 0].tolist())) >= 2          # instances really leave at different iterations
    assert ref["success"].all()
    _assert_same(out, fin, ref, ref_fin, B6, 2)
    assert (out["qp_stats"][:, :, 1, 6] == -1).all()          # nobody hit the cap: the last QP of every step's last solve took no part
    print("slot 0 says \"took no part\" (step-by-step):", (ref["qp_stats"][:, :, 0, 6] == -1).tolist())


@pytest.mark.parametrize("rti", [2, 1])
def test_cap_on_the_iterations_the_last_qp_and_the_pending_reset(rti):
    """The same case with max_sls_iter = 3 and 3 steps: instances 4 and 5 hit the cap in the first solve of every step (success False after 3
    sweeps, as on the oracle).  Such an instance solves the last QP of that solve (slot 1), everyone else has "took no part" there; the steps after the
    failure run on the solver state the failure left behind (_finish_failure's reset is pending).
    qp_stats holds the step's LAST solve.  With rti = 2 that is the second SCP iteration, in which an instance whose first solve failed is masked:
    slsqp_cl_step itself leaves -1 in BOTH its slots there (measured: [-1, -1] for instances 4 and 5), so that the last QP ran can only be read
    off at rti = 1, where the capped solve is the step's last one -- the second parameter; the parity with the step-by-step loop is held at both."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("quadrotor")
    x0 = _spread_x0(m, 0.05)

    def tune(o):
        o.max_sls_iter = 3
    ref, ref_fin = _stepwise(m, 4, B6, 3, x0, rti, tune)
    print("sls_iterations (step-by-step):", ref["sls_iterations"].tolist(), "success:", ref["success"].tolist())
    print("slot 1 status (step-by-step):", ref["qp_stats"][:, :, 1, 6].tolist())
    capped = ~ref["success"][:, 0] & (ref["sls_iterations"][:, 0] == 3)
    assert capped.any()
    if rti == 1:
        assert (ref["qp_stats"][capped, 0, 1, 6] != -1).all()          # the final QP ran for them
    else:
        assert (ref["qp_stats"][capped, 0, :, 6] == -1).all()          # masked in the step's last solve: no QP of it was theirs
    conv = ref["success"][:, 0]
    assert conv.any() and (ref["qp_stats"][conv, 0, 1, 6] == -1).all()          # and for nobody who converged
    out, fin = _persistent(m, 4, B6, 3, x0, rti, tune)
    _assert_same(out, fin, ref, ref_fin, B6, 3)


def test_rocket_odd_tail_of_the_paired_sweep_and_a_failing_instance():
    """Rocket, N = 4 (five sweep columns: the odd tail of the paired first sweep), rti = 2, 2 steps: on the oracle the step-0 counts are 1, 2, 2, 3,
    8, 7 and instances 4 and 5 fail at step 1.  An instance with a failed step leaves the others untouched: they give the bits of a run of their own."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("rocket")
    x0 = _spread_x0(m, 0.15)
    ref, ref_fin = _stepwise(m, 4, B6, 2, x0, 2)
    print("sls_iterations (step-by-step):", ref["sls_iterations"].tolist(), "success:", ref["success"].tolist())
    assert len(set(ref["sls_iterations"][:, 0].tolist())) >= 2
    failed = ~ref["success"].all(axis=1)
    assert failed.any() and not failed.all()
    out, fin = _persistent(m, 4, B6, 2, x0, 2)
    _assert_same(out, fin, ref, ref_fin, B6, 2)
    others = ~failed
    clean, _ = _persistent(m, 4, int(others.sum()), 2, x0[others], 2)
    for k in LOG_KEYS + ("sls_iterations",):
        assert np.array_equal(out[k][others], clean[k], equal_nan=True), k


def test_pendulum_both_loops_data_dependent():
    """Pendulum, N = 5 (six columns), SCP converge mode rti = -1 with scp_eps = 1e-8, 2 steps: the number of solves per step and the iterations of
    every solve are the instance's own.  On the oracle one instance needs 8 iterations in a solve where the others need 1."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    x0 = _spread_x0(m, 0.3)

    def tune(o):
        o.scp_eps = 1e-8
    ref, ref_fin = _stepwise(m, 5, B6, 2, x0, -1, tune)
    print("scp_iterations (step-by-step):", ref["scp_iterations"].tolist(), "sls_iterations:", ref["sls_iterations"].tolist())
    assert len(set(ref["scp_iterations"][:, 0].tolist())) > 1 or len(set(ref["sls_iterations"][:, 0].tolist())) > 1
    out, fin = _persistent(m, 5, B6, 2, x0, -1, tune)
    _assert_same(out, fin, ref, ref_fin, B6, 2)
    assert ref["success"].any()


def test_fewer_waves_than_instances():
    """Case 1 with SLSQP_LOOP_WAVES=2: every wave serves three instances through the queue."""
    m, x0, (ref, ref_fin), _ = _quadrotor_case()
    out, fin = _persistent(m, 4, B6, 2, x0, 2, waves=2)
    _assert_same(out, fin, ref, ref_fin, B6, 2, waves=2)
    assert out["loop_stats"]["waves"] < B6


def test_rocket_with_reference_plant_parameters_and_bounds():
    """The rocket case on the variant with every per-handle option (VAR = REF | PP | BND): a reference row, the default plant parameters given
    explicitly and the model's own box given through set_bounds -- the bits of the step-by-step loop in the same option state."""
    from robust_nonlinear_mpc_amd import get_model, plant_param_defaults
    m = get_model("rocket")
    x0 = _spread_x0(m, 0.15)

    def setup(cl):
        cl.set_reference(np.zeros((1, m.nx)), np.zeros((1, m.nu)))
        cl.set_plant_params(plant_param_defaults(m))
        cl.set_bounds(np.asarray(m.g, dtype=float)[None, :], np.asarray(m.gf, dtype=float)[None, :])
    ref, ref_fin = _stepwise(m, 4, B6, 2, x0, 2, setup=setup)
    assert len(set(ref["sls_iterations"][:, 0].tolist())) >= 2
    out, fin = _persistent(m, 4, B6, 2, x0, 2, setup=setup)
    _assert_same(out, fin, ref, ref_fin, B6, 2)
    assert np.array_equal(out["model_error"], ref["model_error"], equal_nan=True)


def test_the_option_itself():
    """Off: rti_steps = 0 is refused with today's message.  On: precision = 1 and solve_every = 2 are still refused with their reasons; the setter
    rejects 2 and -1 and leaves the getter's value unchanged; with rti_steps = 2 the run equals the option off, bit for bit; after a refusal the
    handle still runs."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model
    L = __import__("robust_nonlinear_mpc_amd")._lib
    m = get_model("pendulum")
    x0 = np.tile(m.extra["x0"], (4, 1))
    cl = ClosedLoopMPC(m, 10, 4)
    lib, f = cl.f.lib, cl.f
    cl.reset(x0)
    assert not f.get_sls_converge() and lib.slsqp_cl_get_sls_converge(f.h) == 0
    f.opts.rti_steps = 0
    assert lib.slsqp_cl_run_scp(f.h, 2, 3, None, L.HOST, C.byref(f.opts)) < 0
    assert "fast-SLS converge mode (rti_steps <= 0) does not run inside the persistent loop (use slsqp_cl_step)" in lib.slsqp_last_error().decode()
    with pytest.raises(RuntimeError, match="rti_steps"):
        cl.run_decoupled(x0, 2)          # persistent_converge defaults to False
    for bad in (2, -1):
        assert lib.slsqp_cl_set_sls_converge(f.h, bad) < 0 and "neither 0 (off) nor 1 (on)" in lib.slsqp_last_error().decode()
        assert lib.slsqp_cl_get_sls_converge(f.h) == 0
        with pytest.raises(RuntimeError):
            f.set_sls_converge(bad)
    f.set_sls_converge(True)
    assert f.get_sls_converge()
    assert lib.slsqp_cl_set_sls_converge(f.h, 2) < 0 and lib.slsqp_cl_set_sls_converge(f.h, -1) < 0 and lib.slsqp_cl_get_sls_converge(f.h) == 1
    cl.reset(x0)
    f.opts.precision = 1
    assert lib.slsqp_cl_run_scp(f.h, 2, 3, None, L.HOST, C.byref(f.opts)) < 0
    assert "precision" in lib.slsqp_last_error().decode()
    f.opts.precision = 0
    f.set_solve_every(2)
    assert lib.slsqp_cl_run_scp(f.h, 2, 3, None, L.HOST, C.byref(f.opts)) < 0
    assert "solve_every = 2" in lib.slsqp_last_error().decode()
    f.set_solve_every(1)
    f.opts.max_sls_iter = 0
    assert lib.slsqp_cl_run_scp(f.h, 2, 3, None, L.HOST, C.byref(f.opts)) < 0
    assert "max_sls_iter >= 1" in lib.slsqp_last_error().decode()
    f.opts.max_sls_iter = 30
    # after the refusals the handle still runs: converge mode, then a fixed number of steps with the option still on
    out = cl.run_decoupled(x0, 2, persistent_converge=True)
    assert out["success"].any() and out["loop_stats"]["mpc_steps"] == 4 * 2 and (out["sls_iterations"] >= 0).all() and out["sls_iterations"].any()
    cl.close()
    cl = ClosedLoopMPC(m, 10, 4)          # (a fresh handle, as the run it is compared with has)
    lib, f = cl.f.lib, cl.f
    assert f.opts.rti_steps == 2
    f.set_sls_converge(True)
    L.check(lib.slsqp_cl_log(f.h, 2))
    cl.reset(x0)
    L.check(lib.slsqp_cl_run_scp(f.h, 2, 3, None, L.HOST, C.byref(f.opts)))
    on = cl._log_result(2, np.zeros((2, 1)), np.zeros((2, 1)), np.zeros((2, 1)))
    on["qp_stats"] = f.get("log_qp_stats", (2, 2, 8), np.int32)
    assert not f.get("log_sls_iterations", (2,), np.int32).any()          # only the new variants write it
    on_fin = _final(cl)
    cl.close()
    cl = ClosedLoopMPC(m, 10, 4)
    off = cl.run_decoupled(x0, 2)
    off_fin = _final(cl)
    cl.close()
    for k in LOG_KEYS + ("qp_stats", "x0_violation"):
        assert np.array_equal(on[k], off[k], equal_nan=True), k
    for k in on_fin:
        assert np.array_equal(on_fin[k], off_fin[k], equal_nan=True), k
    assert "sls_iterations" not in off


def test_quadrotor_against_the_oracle():
    """Case 1 against the CPU restatement of SCP_SLS.solve built on the oracle with fast_SLS.solve's default loop, for the instances whose oracle QPs
    converged: the comparison and tolerances of test_persistent_scp_closed_loop_vs_oracle (tests/test_gpu_cl_scp.py)."""
    from problems import run_oracle_closed_loop
    m, x0, _, (out, _fin) = _quadrotor_case()
    N, steps = 4, 2
    compared = 0
    for b in range(B6):
        ref = run_oracle_closed_loop(m, N, x0[b], steps, 2, None, None)
        if not all(ref["oracle_qp_converged"]):
            continue
        compared += 1
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
    assert compared >= 1


def test_monte_carlo_persistent_converge_equals_the_stepped_monte_carlo():
    """run_monte_carlo(..., persistent=True, persistent_converge=True) on four seeds of a pendulum in fast-SLS converge mode against the default,
    which keeps stepping for this mode."""
    from robust_nonlinear_mpc_amd import get_model, run_monte_carlo
    m = dataclasses.replace(get_model("pendulum"), fast_sls_rti_steps=None)
    N, steps, seeds = 5, 3, np.arange(4)
    x0 = np.asarray(m.extra["x0"], dtype=float)
    ref = run_monte_carlo(m, N, seeds, steps, x0)
    assert "loop_stats" not in ref and "sls_iterations" not in ref          # persistent=None: stepped
    also = run_monte_carlo(m, N, seeds, steps, x0, persistent_converge=True)
    assert "loop_stats" not in also          # the flag alone changes nothing
    out = run_monte_carlo(m, N, seeds, steps, x0, persistent=True, persistent_converge=True)
    assert out["sls_iterations"].shape == (4, steps) and (out["sls_iterations"] >= 1).all() and len(out["loop_stats"]) == 1
    for k in LOG_KEYS + ("x0_violation",):
        assert np.array_equal(out[k], ref[k], equal_nan=True), k
        assert np.array_equal(also[k], ref[k], equal_nan=True), k
    assert ref["success"].any()

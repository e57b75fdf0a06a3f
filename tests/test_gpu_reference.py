"""Reference tracking in the on-device closed loops (slsqp_cl_set_reference): against the CPU restatement of the tracked loop, bit for bit between
the entry points (step by step, persistent, round-based), untouched defaults, the tracked linear cost of slsqp_linearize, the hold of the last row,
the nominal initialiser's tracked KKT point, and the argument checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from reference_cases import case, hessian_diag, oracle_case, ref_window

pytestmark = pytest.mark.gpu

LOG_KEYS = ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x", "backoff_trajectory_u", "success",
            "scp_iterations", "primal_infeasibility", "x0_violation")


def _final(cl):
    m, N = cl.m, cl.N
    return {k: cl.f.get(k, shp) for k, shp in (("x_meas", (m.nx,)), ("nominal_x", (N + 1, m.nx)), ("nominal_u", (N, m.nu)), ("primal_vec", (cl.f.n,)))}


def _make(m, N, B, rti=None, rti_steps=None, reference=None, tune=None):
    from robust_nonlinear_mpc_amd import ClosedLoopMPC
    cl = ClosedLoopMPC(m, N, B, rti=rti, fast_sls_rti_steps=rti_steps, reference=reference)
    if tune:
        tune(cl.f.opts)
    return cl


def _stepwise(cl, steps, x0, W=None, **reset_kw):
    """One slsqp_cl_step per MPC step, qp_stats read after each; closes the handle."""
    L = __import__("robust_nonlinear_mpc_amd")._lib
    L.check(cl.f.lib.slsqp_cl_log(cl.f.h, steps))
    cl.reset(x0, **reset_kw)
    stats = []
    for i in range(steps):
        cl.step(None if W is None else W[i], fetch=False)
        stats.append(cl.f.get("qp_stats", (2, 8), np.int32))
    out = cl._log_result(steps, np.zeros((steps, 1)), np.zeros((steps, 1)), np.zeros((steps, 1)))
    out["qp_stats"] = np.stack(stats, axis=1)
    fin = _final(cl)
    cl.close()
    return out, fin


def _decoupled(cl, steps, x0, W=None, waves=None, **reset_kw):
    """slsqp_cl_run / slsqp_cl_run_scp, optionally with fewer waves than instances; closes the handle."""
    if waves is not None:
        os.environ["SLSQP_LOOP_WAVES"] = str(waves)
    try:
        out = cl.run_decoupled(x0, steps, W, **reset_kw)
    finally:
        os.environ.pop("SLSQP_LOOP_WAVES", None)
    fin = _final(cl)
    cl.close()
    return out, fin


def _assert_same(out, fin, ref, ref_fin, what=""):
    for k in LOG_KEYS + ("qp_stats",):
        assert np.array_equal(out[k], ref[k], equal_nan=True), (what, k)
    for k in fin:
        assert np.array_equal(fin[k], ref_fin[k], equal_nan=True), (what, k)


def _seeded_W(m, B, steps):
    from robust_nonlinear_mpc_amd import disturbance_stream
    return np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)


def _wavy_reference(m, B, T, amp):
    """A time-varying reference that differs per instance: the neutral point plus `amp` sin / cos of (row, instance) on the first three states."""
    Xref = np.tile(np.asarray(m.x_ref, dtype=float), (B, T, 1))
    t, b = np.arange(T)[None, :], np.arange(B)[:, None]
    for i in range(min(3, m.nx)):
        Xref[:, :, i] += amp * np.sin(0.35 * t + 0.7 * b + i)
    Uref = np.tile(np.asarray(m.u_ref, dtype=float), (B, T, 1))
    return Xref, Uref


# ---- A, B: against the CPU restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_tracked_closed_loop_vs_oracle(name):
    """Script settings through run_on_device, per-instance references: state, u0, nominal_x, nominal_u and success against the CPU restatement of the
    tracked loop at the 1e-6 relative of test_persistent_scp_closed_loop_vs_oracle.  A (pendulum): cart-position setpoints 0.5 / -0.5 / 2.0 that
    switch on at row 4, input reference left NULL (= zero).  B (quadrotor): the figure x = 0.3 sin 2t, y = 0.3 (1 - cos 2t) at three heights,
    hover thrust.  The CPU runs differ from the untracked ones by > 1e-3 (tests/test_reference_cpu.py), so 1e-6 separates them."""
    c = case(name)
    m, N, steps, B = c["m"], c["N"], c["steps"], c["B"]
    reference = (c["Xref"], None) if name == "A" else (c["Xref"], c["Uref"])
    cl = _make(m, N, B, reference=reference)
    out = cl.run_on_device(c["x0"], steps)
    cl.close()
    for b in range(B):
        ref = oracle_case(name, b)
        assert ref["success"].all() and ref["oracle_qp_converged"].all()
        scale = max(1.0, np.abs(ref["nominal_x"]).max())
        uscale = max(1.0, np.abs(ref["nominal_u"]).max())
        errs = dict(
            state=np.max(np.abs(out["state_trajectory"][b].T - ref["state"])) / scale,
            u0=np.max(np.abs(out["input_trajectory"][b].T - ref["u0"][: steps - 1])) / max(1.0, np.abs(ref["u0"]).max()),
            nominal_x=np.max(np.abs(out["nominal_trajectory_x"][b].transpose(2, 1, 0) - ref["nominal_x"])) / scale,
            nominal_u=np.max(np.abs(out["nominal_trajectory_u"][b].transpose(2, 1, 0) - ref["nominal_u"])) / uscale)
        print(name, b, errs)
        assert list(out["success"][b]) == list(ref["success"])
        for k, e in errs.items():
            assert e < 1e-6, (b, k, e)


# ---- C: defaults untouched ------------------------------------------------------------------------------------------------------------------
def _c_setup(model):
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    if model == "pendulum":
        N, B, steps = 10, 4, 6
        x0 = np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.1 * np.arange(B)[:, None])
        return m, N, B, steps, x0, None, {}
    N, B, steps = 20, 4, 3
    x0 = np.tile(m.x_ref + 0.3 * (m.extra["x0"] - m.x_ref), (B, 1))
    return m, N, B, steps, x0, _seeded_W(m, B, steps), dict(solve_nominal=True, continuation=2)


@pytest.mark.parametrize("model", ["pendulum", "rocket"])
def test_no_reference_zero_reference_and_cleared_reference_are_the_same_bits(model):
    """A handle that never saw a reference, one with a T = 1 reference of zeros, and one whose reference was set and cleared: identical log arrays,
    qp_stats and final state, step by step and through the persistent launch."""
    m, N, B, steps, x0, W, kw = _c_setup(model)
    rti = 1 if model == "rocket" else None
    rti_steps = 1 if model == "rocket" else None

    def handle(kind):
        cl = _make(m, N, B, rti, rti_steps)
        if kind == "zeros":
            cl.set_reference(np.zeros((1, m.nx)), np.zeros((1, m.nu)))
        elif kind == "cleared":
            cl.set_reference(*_wavy_reference(m, B, 5, 0.3))
            cl.set_reference(None)
        return cl
    for run in (_stepwise, _decoupled):
        ref, ref_fin = run(handle("never"), steps, x0, W, **kw)
        assert ref["success"].any()
        for kind in ("zeros", "cleared"):
            out, fin = run(handle(kind), steps, x0, W, **kw)
            _assert_same(out, fin, ref, ref_fin, (run.__name__, kind))


# ---- D: slsqp_linearize ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N", [("pendulum", 10), ("quadrotor", 20), ("rocket", 20)])
def test_linearize_forms_the_tracked_linear_cost_and_nothing_else(model, N):
    """q = 2 Hd (y - y_ref) as numpy forms it, bit for bit, with a per-instance reference shorter than the horizon (rows held); A, Bm, c, g, gN keep
    the bits of a handle without a reference."""
    from robust_nonlinear_mpc_amd import BatchedFastSLS, get_model
    m = get_model(model)
    B, T = 2, 7
    rng = np.random.default_rng(5)
    X = m.x_ref + 0.05 * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, (B, N + 1, m.nx))
    U = m.u_ref + 0.05 * (m.u_ub - m.u_lb) * rng.uniform(-1, 1, (B, N, m.nu))
    Xref = m.x_ref + 0.1 * rng.uniform(-1, 1, (B, T, m.nx))
    Uref = m.u_ref + 0.1 * rng.uniform(-1, 1, (B, T, m.nu))
    shapes = dict(A=(N, m.nx, m.nx), Bm=(N, m.nx, m.nu), c=(N, m.nx), g=(N, m.ni), gN=(m.ni_f,), q=(m.n_var(N),))
    got = {}
    for kind in ("plain", "tracked"):
        f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=B)
        if kind == "tracked":
            f.set_reference(Xref, Uref)
        f.linearize(X, U)
        got[kind] = {k: f.get(k, s) for k, s in shapes.items()}
        f.close()
    Hd = hessian_diag(m, N)
    for b in range(B):
        y = np.concatenate([np.concatenate([X[b, k], U[b, k]]) for k in range(N)] + [X[b, N]])
        assert np.array_equal(got["tracked"]["q"][b], 2.0 * Hd * (y - ref_window(Xref[b], Uref[b], 0, N))), b
        assert np.array_equal(got["plain"]["q"][b], 2.0 * Hd * y), b
    assert not np.array_equal(got["tracked"]["q"], got["plain"]["q"])
    for k in ("A", "Bm", "c", "g", "gN"):
        assert np.array_equal(got["tracked"][k], got["plain"][k]), k


def test_linearize_uses_the_window_of_the_handles_step_count():
    """After two slsqp_cl_step the handle is at MPC step 2: slsqp_linearize reads rows min(2 + k, T - 1); slsqp_cl_init restarts at row 0."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, T = 10, 2, 9
    Xref, Uref = _wavy_reference(m, B, T, 0.2)
    cl = _make(m, N, B, reference=(Xref, Uref))
    x0 = np.tile(m.extra["x0"], (B, 1))
    cl.reset(x0)
    cl.step(None, fetch=False)
    cl.step(None, fetch=False)
    X, U = cl.f.get("nominal_x", (N + 1, m.nx)), cl.f.get("nominal_u", (N, m.nu))
    Hd = hessian_diag(m, N)
    y = [np.concatenate([np.concatenate([X[b, k], U[b, k]]) for k in range(N)] + [X[b, N]]) for b in range(B)]
    cl.f.linearize(X, U)
    q = cl.f.get("q", (cl.f.n,))
    for b in range(B):
        assert np.array_equal(q[b], 2.0 * Hd * (y[b] - ref_window(Xref[b], Uref[b], 2, N))), b
    cl.reset(x0)
    cl.f.linearize(X, U)
    q = cl.f.get("q", (cl.f.n,))
    for b in range(B):
        assert np.array_equal(q[b], 2.0 * Hd * (y[b] - ref_window(Xref[b], Uref[b], 0, N))), b
    cl.close()


# ---- E: the persistent loops under a time-varying, per-instance reference -----------------------------------------------------------------
def _tune_converge(o):
    o.scp_eps = 1e-8


@pytest.mark.parametrize("model,N,B,steps,waves,rti,rti_steps,tune", [
    ("rocket", 20, 96, 6, 7, 1, 1, None),
    ("pendulum", 10, 50, 8, 7, None, None, None),
    ("pendulum", 10, 8, 2, None, -1, 2, _tune_converge),
])
def test_persistent_loops_are_bitwise_the_step_by_step_loop_with_a_reference(model, N, B, steps, waves, rti, rti_steps, tune):
    """Inside the persistent launches every instance is at its own MPC step -- with 7 waves for 96 or 50 instances they are at different steps at the
    same time and change hands -- so the window of the reference must come from the instance's own step count.  Rocket: rti 1 / one fast-SLS step
    (k_cl_loop), also through the round-based loop; pendulum: the script setting and SCP converge mode (k_cl_loop_scp)."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    reference = _wavy_reference(m, B, steps + 4, 0.2)      # shorter than steps + N + 1: the hold is part of every window near the end
    if model == "rocket":
        x0, kw = np.tile(m.x_ref + 0.3 * (m.extra["x0"] - m.x_ref), (B, 1)), dict(solve_nominal=True, continuation=2)
    else:
        x0, kw = np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.2 * np.random.default_rng(3).uniform(-1, 1, (B, 1))), {}
    W = _seeded_W(m, B, steps)
    ref, ref_fin = _stepwise(_make(m, N, B, rti, rti_steps, reference, tune), steps, x0, W, **kw)
    print("success rate", ref["success"].mean())
    assert ref["success"].any()
    out, fin = _decoupled(_make(m, N, B, rti, rti_steps, reference, tune), steps, x0, W, waves=waves, **kw)
    _assert_same(out, fin, ref, ref_fin, "persistent")
    assert out["loop_stats"]["waves"] == (B if waves is None else waves)
    plain, _ = _decoupled(_make(m, N, B, rti, rti_steps, None, tune), steps, x0, W, waves=waves, **kw)
    assert not np.array_equal(plain["nominal_trajectory_x"], out["nominal_trajectory_x"])      # the reference is in use
    if model == "rocket":
        def rounds(o):
            o.cl_persistent = 0
        out, fin = _decoupled(_make(m, N, B, rti, rti_steps, reference, rounds), steps, x0, W, **kw)
        _assert_same(out, fin, ref, ref_fin, "rounds")


# ---- F: hold and setpoint -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [_stepwise, _decoupled])
def test_last_row_is_held(run):
    """T = 1 against T = steps + N + 1 equal rows, and T = 3 against the same rows padded by hand with the last one: the same bits."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, steps = 10, 3, 5
    x0 = np.tile(m.extra["x0"], (B, 1))
    sp = np.zeros((B, 1, m.nx)); sp[:, 0, 0] = (0.5, -0.5, 1.0)
    usp = np.full((B, 1, m.nu), 0.1)
    short = np.zeros((B, 3, m.nx)); short[:, :, 0] = np.array([[0.1, 0.2, 0.4], [-0.1, -0.3, -0.2], [0.0, 0.5, 1.0]])
    ushort = np.zeros((B, 3, m.nu))
    Tfull = steps + N + 1
    pairs = [((sp, usp), (np.repeat(sp, Tfull, axis=1), np.repeat(usp, Tfull, axis=1))),
             ((short, ushort), (np.concatenate([short, np.repeat(short[:, -1:], Tfull - 3, axis=1)], axis=1), np.zeros((B, Tfull, m.nu))))]
    for a, b in pairs:
        ref, ref_fin = run(_make(m, N, B, reference=a), steps, x0)
        out, fin = run(_make(m, N, B, reference=b), steps, x0)
        assert ref["success"].any()
        _assert_same(out, fin, ref, ref_fin, run.__name__)


# ---- G: the initialiser ---------------------------------------------------------------------------------------------------------------------
def _nlp_kkt_residual_tracked(m, N, X, U, x_meas, y_ref):
    """The certificate of tests/test_gpu_parity.py::_nlp_kkt_residual for the tracked cost: dynamics defect, box violation and
    min over multipliers (nu free, lambda >= 0 on active bounds) of |2 Hd (y - y_ref) + J' nu +- lambda|, relative."""
    from scipy.optimize import lsq_linear
    from problems import host_jac
    nx, nz, mid = m.nx, m.nz, m.model_id
    n = nz * N + nx
    y = np.concatenate([np.concatenate([X[k], U[k]]) for k in range(N)] + [X[N]])
    grad = 2.0 * hessian_diag(m, N) * (y - y_ref)
    hi = np.concatenate([np.concatenate([m.x_ub, m.u_ub])] * N + [m.x_ub])
    lo = np.concatenate([np.concatenate([m.x_lb, m.u_lb])] * N + [m.x_lb])
    J = np.zeros((nx * (N + 1), n))
    J[:nx, :nx] = np.eye(nx)
    defect = np.abs(X[0] - x_meas).max()
    for k in range(N):
        A, Bm, f = host_jac(mid, X[k], U[k])
        r = nx * (k + 1)
        J[r:r + nx, k * nz:k * nz + nx] = A
        J[r:r + nx, k * nz + nx:(k + 1) * nz] = Bm
        J[r:r + nx, (k + 1) * nz:(k + 1) * nz + nx] = -np.eye(nx)
        defect = max(defect, np.abs(f - X[k + 1]).max())
    viol = max(np.maximum(y[nx:] - hi[nx:], 0).max(), np.maximum(lo[nx:] - y[nx:], 0).max())
    act_u = np.where((np.abs(y - hi) < 1e-7) & (np.arange(n) >= nx))[0]
    act_l = np.where((np.abs(y - lo) < 1e-7) & (np.arange(n) >= nx))[0]
    M = np.hstack([J.T, np.eye(n)[:, act_u], -np.eye(n)[:, act_l]])
    lb = np.concatenate([-np.inf * np.ones(J.shape[0]), np.zeros(len(act_u) + len(act_l))])
    sol = lsq_linear(M, -grad, bounds=(lb, np.inf * np.ones(M.shape[1])), tol=1e-14, max_iter=500)
    return defect, viol, np.abs(M @ sol.x + grad).max() / max(1.0, np.abs(grad).max())


@pytest.mark.parametrize("model,N", [("pendulum", 10), ("quadrotor", 20)])
def test_nominal_initialiser_reaches_the_kkt_point_of_the_tracked_cost(model, N):
    """reset(solve_nominal=True) with a setpoint reference: the first nominal satisfies the KKT conditions of the NLP with the TRACKED cost, certified
    on the host with the thresholds of test_nominal_initialiser_reaches_nlp_kkt_point -- and the same point fails the certificate of the untracked
    cost (y_ref = 0), so the test cannot pass on the cost around the origin."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    B = 3
    Xref = np.tile(np.asarray(m.x_ref, dtype=float), (B, 1, 1))
    Xref[:, 0, 0] = (0.5, -0.5, 1.0)
    Uref = np.tile(np.asarray(m.u_ref, dtype=float), (B, 1, 1))
    if model == "pendulum":
        x0 = np.tile(m.extra["x0"], (B, 1))
    else:
        Xref[:, 0, 2] = (0.3, 0.0, -0.3)
        x0 = np.stack([m.x_ref + 0.05 * (m.x_ub - m.x_lb) * np.random.default_rng(40 + b).uniform(-1, 1, m.nx) for b in range(B)])
        x0[:, 6:10] /= np.linalg.norm(x0[:, 6:10], axis=1, keepdims=True)
    cl = _make(m, N, B, reference=(Xref, Uref))
    cl.reset(x0, solve_nominal=True)
    X, U = cl.f.get("nominal_x", (N + 1, m.nx)), cl.f.get("nominal_u", (N, m.nu))
    st, its = cl.nlp_status, cl.nlp_iterations
    cl.close()
    for b in range(B):
        y_ref = ref_window(Xref[b], Uref[b], 0, N)
        defect, viol, stat = _nlp_kkt_residual_tracked(m, N, X[b], U[b], x0[b], y_ref)
        _, _, stat0 = _nlp_kkt_residual_tracked(m, N, X[b], U[b], x0[b], np.zeros_like(y_ref))
        print(model, b, "nlp_status", st[b], "iterations", its[b], "defect", defect, "box", viol, "stationarity", stat, "with y_ref = 0", stat0)
        assert defect < 1e-6 and viol < 1e-8, (b, defect, viol)
        assert stat < 1e-5, (b, stat)
        assert stat0 > 1e-3, (b, stat0)


# ---- Monte-Carlo driver ---------------------------------------------------------------------------------------------------------------------
def test_monte_carlo_cuts_a_per_seed_reference_with_the_seeds():
    """run_monte_carlo(reference=...): a per-seed reference in one slice and cut into two slices gives the same bits, differs from the untracked
    run, and "neutral" is the setpoint (x_ref, u_ref)."""
    from robust_nonlinear_mpc_amd import get_model, run_monte_carlo
    m = get_model("quadrotor")
    N, S, steps = 10, 5, 3
    x0 = m.x_ref + 0.02 * (m.x_ub - m.x_lb)
    x0[6:10] /= np.linalg.norm(x0[6:10])
    reference = _wavy_reference(m, S, steps + 3, 0.1)
    kw = dict(noise=True, gather=False)
    one = run_monte_carlo(m, N, np.arange(S), steps, x0, reference=reference, **kw)
    two = run_monte_carlo(m, N, np.arange(S), steps, x0, reference=reference, slices=2, **kw)
    plain = run_monte_carlo(m, N, np.arange(S), steps, x0, **kw)
    assert one["success"].any()
    for k in LOG_KEYS:
        assert np.array_equal(one[k], two[k], equal_nan=True), k
    assert not np.array_equal(one["nominal_trajectory_x"], plain["nominal_trajectory_x"])
    a = run_monte_carlo(m, N, np.arange(S), steps, x0, reference="neutral", **kw)
    b = run_monte_carlo(m, N, np.arange(S), steps, x0, reference=(m.x_ref[None, :], m.u_ref[None, :]), **kw)
    for k in LOG_KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert not np.array_equal(a["nominal_trajectory_x"], plain["nominal_trajectory_x"])


# ---- H: argument checks ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_leave_the_reference_in_force():
    from robust_nonlinear_mpc_amd import BatchedFastSLS, get_model
    L = __import__("robust_nonlinear_mpc_amd")._lib
    m = get_model("pendulum")
    N, B, T = 10, 2, 4
    f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=B)
    rng = np.random.default_rng(1)
    X, U = 0.1 * rng.uniform(-1, 1, (B, N + 1, m.nx)), 0.1 * rng.uniform(-1, 1, (B, N, m.nu))
    Xref, Uref = rng.uniform(-1, 1, (B, T, m.nx)), rng.uniform(-1, 1, (B, T, m.nu))
    f.set_reference(Xref, Uref)

    def q_now():
        f.linearize(X, U)
        return f.get("q", (f.n,))
    q_ref = q_now()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = Xref.copy(); bad[1, 2, 0] = np.nan
    inf = Uref.copy(); inf[0, 0, 0] = np.inf
    for args, word in (((ptr(Xref), ptr(Uref), -1, 1), "T"), ((ptr(bad), ptr(Uref), T, 1), "NaN"), ((ptr(Xref), ptr(inf), T, 1), "infinite"),
                       ((ptr(Xref), ptr(Uref), T, 2), "per_instance"), ((ptr(Xref), ptr(Uref), T, -1), "per_instance"),
                       ((ptr(Xref), None, 0, 0), "T"), ((None, None, T, 0), "Xref")):
        assert f.lib.slsqp_cl_set_reference(f.h, *args, L.HOST) < 0, args
        assert word in f.lib.slsqp_last_error().decode(), (word, f.lib.slsqp_last_error().decode())
        assert np.array_equal(q_now(), q_ref), args
    with pytest.raises(ValueError):
        f.set_reference(np.zeros((B + 1, T, m.nx)))
    with pytest.raises(ValueError):
        f.set_reference(np.zeros((T, m.nx)), np.zeros((T + 1, m.nu)))
    assert np.array_equal(q_now(), q_ref)
    # shared reference, NULL input reference, then cleared
    f.set_reference(Xref[0])
    y = np.concatenate([np.concatenate([X[1, k], U[1, k]]) for k in range(N)] + [X[1, N]])
    assert np.array_equal(q_now()[1], 2.0 * hessian_diag(m, N) * (y - ref_window(Xref[0], np.zeros((T, m.nu)), 0, N)))
    f.set_reference(None)
    assert np.array_equal(q_now()[1], 2.0 * hessian_diag(m, N) * y)
    f.close()


def test_setter_under_debug_allocators():
    """slsqp_cl_set_reference with shared and per-instance host buffers of exactly the documented sizes, in a child process whose allocators check
    their block boundaries (as tests/test_gpu_multiwave.py::test_new_entry_points_under_debug_allocators)."""
    env = dict(os.environ, MALLOC_CHECK_="3", PYTHONMALLOC="malloc_debug")
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.join(ROOT, "tests", "abi_memcheck_reference.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "abi_memcheck_reference ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

"""Hold steps on the device (slsqp_cl_hold_step, k_cl_hold): every hold step against the numpy restatement tests/hold_ref.py from the state fetched
right before it (so no error accumulates across steps), on both stores of the gains (K and the compact Kc) and up to k = N - 1; solve_every = 1 is
today's loop bit for bit; the solve after holds starts from the measured state and reads the reference / bounds rows of the step count the holds
advanced; plant parameters; an instance without a valid plan; the refusals; a rerun.

Tolerances: u0 and hold_xi 1e-11 max(1, |.|inf) (summation order over at most 64 x 17 terms, times 100); x_meas after the plant step 1e-12, what
tests/test_gpu_plant_params.py allows one plant step against the host's dynamics."""
import numpy as np
import pytest

import hold_ref as HR
import plant_params_helpers as H

pytestmark = pytest.mark.gpu

TOL_POLICY, TOL_PLANT = 1e-11, 1e-12


def _lib():
    return __import__("robust_nonlinear_mpc_amd")._lib


def _make(m, N, B, rti=None, rti_steps=None, **kw):
    from robust_nonlinear_mpc_amd import ClosedLoopMPC
    return ClosedLoopMPC(m, N, B, rti=rti, fast_sls_rti_steps=rti_steps, **kw)


def _x0(m, B, scale=0.3):
    """Per-instance initial states around the script's (pendulum, rocket) or near the neutral point (quadrotor)."""
    rng = np.random.default_rng(21)
    if m.name == "quadrotor":
        x0 = m.x_ref + 0.02 * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, (B, m.nx))
        x0[:, 6:10] /= np.linalg.norm(x0[:, 6:10], axis=1, keepdims=True)
        return x0
    s = scale if m.name == "rocket" else 1.0
    return m.x_ref + s * (m.extra["x0"] - m.x_ref) * (1.0 + 0.1 * rng.uniform(-1, 1, (B, 1)))


def _seeded_W(m, B, steps):
    from robust_nonlinear_mpc_amd import disturbance_stream
    return np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)


def _pre(cl):
    m, N, f = cl.m, cl.N, cl.f
    return dict(x_meas=f.get("x_meas", (m.nx,)), nominal_x=f.get("nominal_x", (N + 1, m.nx)), nominal_u=f.get("nominal_u", (N, m.nu)),
                K=f.get("K", (N, N + 1, m.nu, m.nx)), A=f.get("A", (N, m.nx, m.nx)), Bm=f.get("Bm", (N, m.nx, m.nu)), hold_xi=f.get("hold_xi", (N + 1, m.nx)),
                success=f.get("scp_success", (), np.int32))


def _post(cl):
    m, N, f = cl.m, cl.N, cl.f
    return dict(u0=f.get("u0", (m.nu,)), x_meas=f.get("x_meas", (m.nx,)), hold_xi=f.get("hold_xi", (N + 1, m.nx)), hold_index=f.get("hold_index", (), np.int32),
                hold_policy=f.get("hold_policy", (), np.int32), nominal_x=f.get("nominal_x", (N + 1, m.nx)), nominal_u=f.get("nominal_u", (N, m.nu)))


def _close(a, b, tol):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= tol * max(1.0, np.abs(b).max())


# ---- 1: every hold step against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,rti,rti_steps,N,B,M,steps", [
    ("pendulum", 3, 2, 4, 5, 3, 7), ("quadrotor", 3, 2, 3, 3, 2, 4),
    ("rocket", 1, 1, 4, 3, 4, 5),       # the gains stay in the compact store Kc; k reaches N - 1
    ("rocket", 1, 1, 4, 70, 2, 3),      # more than one block of the shift kernel
])
def test_every_hold_step_is_the_restatement(model, rti, rti_steps, N, B, M, steps):
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    cl = _make(m, N, B, rti, rti_steps)
    cl.reset(x0)
    states, inputs, held = [], [], 0
    worst = dict(u0=0.0, xi=0.0, x=0.0)
    for i in range(steps):
        k = i % M
        if k == 0:
            states.append(cl.f.get("x_meas", (m.nx,)))
            cl.step(W[i], fetch=False)
            inputs.append(cl.f.get("u0", (m.nu,)))
            assert not cl.f.get("hold_index", (), np.int32).any()      # a solve sets the index back
            continue
        p = _pre(cl)
        states.append(p["x_meas"])
        cl.hold_step(W[i], fetch=False)
        q = _post(cl)
        inputs.append(q["u0"])
        held += 1
        assert (q["hold_index"] == k).all() and np.array_equal(q["hold_policy"], p["success"])
        assert np.array_equal(q["nominal_x"][:, :N], p["nominal_x"][:, 1:]) and np.array_equal(q["nominal_u"][:, :N - 1], p["nominal_u"][:, 1:])      # the one-stage shift; u is not written into the plan
        assert np.array_equal(q["nominal_u"][:, N - 1], p["nominal_u"][:, N - 1])
        if k > 1:
            assert not p["hold_xi"][:, 0].any() and not p["hold_xi"][:, k:].any()
        for b in range(B):
            xi0 = p["hold_xi"][b] if k > 1 else np.zeros((N + 1, m.nx))      # (a new plan starts from no columns, whatever the last one left)
            u, xn, xi = HR.hold_step(m.model_id, k, p["x_meas"][b], p["nominal_x"][b, 1], p["nominal_u"][b, 1], xi0, p["A"][b], p["Bm"][b], p["K"][b],
                                     E=m.E, w=W[i][b], hold_policy=int(p["success"][b]))
            worst["u0"] = max(worst["u0"], np.abs(q["u0"][b] - u).max() / max(1.0, np.abs(u).max()))
            worst["xi"] = max(worst["xi"], np.abs(q["hold_xi"][b] - xi).max() / max(1.0, np.abs(xi).max()))
            # the plant step from the DEVICE's input, so that the policy's rounding does not count against the plant
            _, xn_dev, _ = HR.hold_step(m.model_id, k, p["x_meas"][b], p["x_meas"][b], q["u0"][b], xi0, p["A"][b], p["Bm"][b], p["K"][b], E=m.E, w=W[i][b], hold_policy=0)
            worst["x_policy"] = max(worst.get("x_policy", 0.0), np.abs(q["x_meas"][b] - xn).max())      # (printed only: the restatement's own input instead)
            worst["x"] = max(worst["x"], np.abs(q["x_meas"][b] - xn_dev).max())
            assert _close(q["u0"][b], u, TOL_POLICY) and _close(q["hold_xi"][b], xi, TOL_POLICY), (i, b, worst)
            assert np.abs(q["x_meas"][b] - xn_dev).max() < TOL_PLANT, (i, b, worst)
            if p["success"][b]:
                assert not q["hold_xi"][b, 0].any() and not q["hold_xi"][b, k + 1:].any()      # rows above the index are zero
                fb = np.abs(q["u0"][b] - p["nominal_u"][b, 1]).max()
                worst["feedback_min"], worst["feedback_max"] = min(worst.get("feedback_min", np.inf), fb), max(worst.get("feedback_max", 0.0), fb)
                assert fb > 1e-9               # the feedback acts (noise W)
    print(model, (rti, rti_steps), "N", N, "B", B, "M", M, "hold steps", held, "worst", worst)
    assert held == steps - (steps + M - 1) // M and cl.f.get("scp_success", (), np.int32).any()
    succ_all = cl.f.get("scp_success", (), np.int32)
    cl.close()
    # the same run without a fetch of K in between (the compact gains are then read where they lie): the same bits, and the log's entries
    cl2 = _make(m, N, B, rti, rti_steps, solve_every=M)
    out = cl2.run_on_device(x0, steps, W)
    assert np.array_equal(cl2.f.get("scp_success", (), np.int32), succ_all)
    cl2.close()
    assert np.array_equal(out["input_trajectory"], np.stack(inputs, axis=2)[:, :, :steps - 1])
    hold_at = np.arange(steps) % M != 0
    assert np.array_equal(out["state_trajectory"][:, :, hold_at], np.stack(states, axis=2)[:, :, hold_at])
    assert np.array_equal(out["hold_index"], np.tile(np.arange(steps) % M, (B, 1)))
    assert not out["scp_iterations"][:, hold_at].any() and not out["x0_violation"][:, hold_at].any()
    for i in np.nonzero(hold_at)[0]:      # back-offs and success of a hold step's entry are the last solve's
        assert np.array_equal(out["backoff_trajectory_x"][..., i], out["backoff_trajectory_x"][..., i - i % M]) and np.array_equal(out["success"][:, i], out["success"][:, i - i % M])
        assert np.array_equal(out["hold_policy"][:, i], out["success"][:, i])


# ---- 2: solve_every = 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,B", [("pendulum", 4, 5), ("rocket", 4, 3)])
def test_solve_every_one_is_todays_loop(model, N, B):
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    steps = 4
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    outs = []
    for ctor, call in (({}, {}), (dict(solve_every=1), {}), ({}, dict(solve_every=1)), (dict(solve_every=2), dict(solve_every=1))):
        cl = _make(m, N, B, **ctor)
        outs.append(cl.run_on_device(x0, steps, W, **call))
        outs[-1]["final_x"] = cl.f.get("x_meas", (m.nx,))
        assert not cl.f.get("hold_index", (), np.int32).any() and not cl.f.get("hold_xi", (N + 1, m.nx)).any() and not cl.f.get("hold_policy", (), np.int32).any()
        cl.close()
    for o in outs[1:]:
        assert set(o) == set(outs[0]) and "hold_index" not in o and "hold_policy" not in o
        for k in o:
            if not k.startswith("t_"):
                assert np.array_equal(o[k], outs[0][k], equal_nan=True), k


# ---- 3: the solve after holds -----------------------------------------------------------------------------------------------------------------------
def test_solve_after_holds_starts_from_the_measured_state():
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, M, steps = 4, 5, 3, 7
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    cl = _make(m, N, B)
    cl.reset(x0)
    seen = 0
    for i in range(steps):
        if i % M:
            cl.hold_step(W[i], fetch=False)
            continue
        xm = cl.f.get("x_meas", (m.nx,))
        r = cl.step(W[i])
        if i == 0:
            continue
        ok = r["success"]
        assert ok.any()
        assert np.array_equal(r["nominal_x"][ok, 0], xm[ok])      # stage 0 of the solved plan is the measured state, as in a plain loop
        want = np.maximum(xm - m.x_ub, m.x_lb - xm).max(axis=1) - 1e-10      # (every bound row of the QP carries the 1e-10 pad, tests/test_gpu_bounds.py)
        print("step", i, "x0_violation", r["x0_violation"][:, 0], "want", want)
        assert np.abs(r["x0_violation"][:, 0] - want).max() < 1e-12
        seen += 1
    assert seen == 2
    cl.close()


def test_reference_and_bounds_windows_read_the_row_of_the_step_count():
    """A per-instance reference and per-instance bounds with T > 1 rows that all differ.  After one solved step and two hold steps the handle's step
    count is 3: the next solved step (one SCP iteration, so q and g are those of its only linearisation, at the shifted nominal) forms
    q = 2 H (y_nom - window 3) and g_k = row (3 + k) - G [x_k; u_k]; the windows of any other step miss by more than 1e-4."""
    import reference_cases as RC
    from bounds_cases import bounds_window
    from problems import host_ddyn
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, T = 4, 3, 12
    t, bb = np.arange(T)[None, :], np.arange(B)[:, None]
    Xref = np.tile(np.asarray(m.x_ref, dtype=float), (B, T, 1))
    Xref[:, :, 0] += 0.05 * np.sin(0.35 * t + 0.7 * bb)
    Uref = np.tile(np.asarray(m.u_ref, dtype=float), (B, T, 1)) + 0.01 * np.cos(0.5 * t + bb)[:, :, None]
    g = np.tile(m.g, (B, T, 1)) * (1.0 - 0.05 * (0.5 + 0.5 * np.sin(0.35 * t + 0.7 * bb))[:, :, None])
    gf = np.tile(m.gf, (B, T, 1)) * (1.0 - 0.05 * (0.5 + 0.5 * np.cos(0.3 * t + bb))[:, :, None])
    x0, W = _x0(m, B), _seeded_W(m, B, 4)
    cl = _make(m, N, B, 1, 1, reference=(Xref, Uref), bounds=(g, gf))
    cl.reset(x0)
    cl.step(W[0], fetch=False)
    cl.hold_step(W[1], fetch=False)
    cl.hold_step(W[2], fetch=False)
    X, U = cl.f.get("nominal_x", (N + 1, m.nx)), cl.f.get("nominal_u", (N, m.nu))
    cl.step(W[3], fetch=False)
    q, gk, gN = cl.f.get("q", (cl.f.n,)), cl.f.get("g", (N, m.ni)), cl.f.get("gN", (m.ni_f,))
    cl.close()
    Hd = RC.hessian_diag(m, N)
    for b in range(B):
        Xs = np.vstack([X[b, 1:], host_ddyn(m.model_id, X[b, N], U[b, N - 1])[None]])      # the shift slsqp_cl_step applies at its top
        Us = np.vstack([U[b, 1:], U[b, N - 1:]])
        y = np.concatenate([np.concatenate([Xs[k], Us[k]]) for k in range(N)] + [Xs[N]])
        err = {}
        for s in range(6):
            gw, gfw = bounds_window(g[b], gf[b], s, N)
            want_g = np.stack([gw[k] - m.G @ np.concatenate([Xs[k], Us[k]]) for k in range(N)])
            err[s] = max(np.abs(q[b] - 2.0 * Hd * (y - RC.ref_window(Xref[b], Uref[b], s, N))).max(), np.abs(gk[b] - want_g).max(), np.abs(gN[b] - (gfw - m.Gf @ Xs[N])).max())
        print("instance", b, "error by window", err)
        assert err[3] < 1e-9 and min(v for s, v in err.items() if s != 3) > 1e-4, (b, err)


# ---- 4: plant parameters ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,B", [("pendulum", 4, 4), ("rocket", 4, 3)])
def test_hold_step_plant_uses_the_parameters(model, N, B):
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    P = H.spread_params(m, B, 20.0, seed=5)
    P[0] = H.host_defaults(m.model_id)      # a row of defaults: the model's own step, error exactly 0
    x0, W = _x0(m, B), _seeded_W(m, B, 3)
    cl = _make(m, N, B, plant_params=P)
    _lib().check(cl.f.lib.slsqp_cl_log(cl.f.h, 3))
    cl.reset(x0)
    cl.step(W[0], fetch=False)
    for i in (1, 2):
        xm = cl.f.get("x_meas", (m.nx,))
        cl.hold_step(W[i], fetch=False)
        u0, xn, me = cl.f.get("u0", (m.nu,)), cl.f.get("x_meas", (m.nx,)), cl.f.get("model_err", (m.nx,))
        assert np.array_equal(cl.f.get("log_model_error", (3, m.nx))[:, i], me)
        assert not me[0].any()
        for b in range(B):
            fp, fc = H.host_ddyn_p(m.model_id, xm[b], u0[b], P[b]), H.host_ddyn_c(m.model_id, xm[b], u0[b])
            e_m, e_x = np.abs(me[b] - (fp - fc)).max(), np.abs(xn[b] - (fp + m.E @ W[i][b])).max()
            print(model, i, b, "model_err err", e_m, "x_meas err", e_x, "|model_err|", np.abs(fp - fc).max())
            assert e_m < TOL_PLANT and e_x < TOL_PLANT, (i, b, e_m, e_x)
            assert b == 0 or np.abs(fp - fc).max() > 1e-6      # the parameters reach the step
    cl.close()


# ---- 5: an instance without a valid plan ------------------------------------------------------------------------------------------------------------
def test_failed_instance_applies_the_nominal_input_and_the_others_do_not_notice():
    """Before MPC step 2, instance 1 gets rows whose row 2 puts the upper bound of its cart position 1e-3 below its measured state (the device of
    tests/test_gpu_bounds.py::test_stage0_gate_reads_the_rows_of_the_steps_own_window): under the strict gate its solve is refused.  The hold steps
    that follow give it the shifted nominal input and hold_policy = 0; the other instances have the bits of a batch without the offset."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B = 6, 4
    x0 = np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.1 * np.arange(B)[:, None])
    W = _seeded_W(m, B, 5)

    def run(exclude):
        cl = _make(m, N, B, 1, 1, bounds=(m.g[None, :], m.gf[None, :]))
        cl.reset(x0)
        cl.step(W[0], fetch=False)
        cl.step(W[1], fetch=False)
        xm = cl.f.get("x_meas", (m.nx,))
        if exclude:
            g = np.tile(m.g, (B, 4, 1))
            g[1, 2, 0] = xm[1, 0] - 1e-3
            cl.set_bounds(g)
        r = [cl.step(W[2])]
        for i in (3, 4):
            r.append(cl.hold_step(W[i]))
            r[-1]["hold_xi"] = cl.f.get("hold_xi", (N + 1, m.nx))
        cl.close()
        return r
    ref, out = run(False), run(True)
    assert ref[0]["success"].all() and not out[0]["success"][1] and out[0]["success"][[0, 2, 3]].all()
    for h_ref, h_out in zip(ref[1:], out[1:]):
        assert h_ref["hold_policy"].all() and list(h_out["hold_policy"]) == [True, False, True, True]
        assert np.array_equal(h_out["u0"][1], h_out["nominal_u"][1, 0]) and not h_out["hold_xi"][1].any()      # the shifted nominal input; no columns
        assert not np.array_equal(h_ref["u0"][1], h_ref["nominal_u"][1, 0])
        for k in ("u0", "x_next", "state", "nominal_x", "nominal_u", "backoff_x", "backoff_u", "hold_xi", "hold_index"):
            assert np.array_equal(h_out[k][[0, 2, 3]], h_ref[k][[0, 2, 3]]), k


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refused_hold_steps_change_nothing():
    """Hold before any solve; the N-th hold in a row; hold after slsqp_cl_run: each raises with the library's message and leaves x_meas, the nominal and
    the step count as they were -- the logged run with the refused calls in it has the bits of the run without them (a step count that had moved
    would shift every later log entry and window)."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, steps = 4, 3, 6
    x0, W = _x0(m, B), _seeded_W(m, B, steps)

    def state(cl):
        mm, NN = cl.m, cl.N
        return [cl.f.get(k, s) for k, s in (("x_meas", (mm.nx,)), ("nominal_x", (NN + 1, mm.nx)), ("nominal_u", (NN, mm.nu)), ("u0", (mm.nu,)), ("hold_xi", (NN + 1, mm.nx)))]

    def refused(cl, word):
        before = state(cl) + [cl.f.get("hold_index", (), np.int32)]
        with pytest.raises(RuntimeError, match=word):
            cl.f.hold_step(None)
        after = state(cl) + [cl.f.get("hold_index", (), np.int32)]
        assert all(np.array_equal(a, b) for a, b in zip(before, after))

    def run(with_refusals):
        cl = _make(m, N, B)
        _lib().check(cl.f.lib.slsqp_cl_log(cl.f.h, steps))
        cl.reset(x0)
        if with_refusals:
            refused(cl, "no slsqp_cl_step since slsqp_cl_init")
        cl.step(W[0], fetch=False)
        for i in (1, 2, 3):
            cl.hold_step(W[i], fetch=False)
        if with_refusals:
            refused(cl, "at most N - 1 hold steps")
            with pytest.raises(RuntimeError, match="loc must be"):
                _lib().check(cl.f.lib.slsqp_cl_hold_step(cl.f.h, None, 7))
        cl.step(W[4], fetch=False)
        cl.hold_step(W[5], fetch=False)
        out = cl._log_result(steps, np.zeros((steps, 1)), np.zeros((steps, 1)), np.zeros((steps, 1)))
        out["hold_index"] = cl.f.get("log_hold", (steps,), np.int32)
        out["final"] = np.concatenate([a.ravel() for a in state(cl)])
        cl.close()
        return out
    a, b = run(True), run(False)
    assert list(a["hold_index"][0]) == [0, 1, 2, 3, 0, 1]
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    # after a persistent run there is no per-batch plan
    mr = get_model("rocket")
    Wr = _seeded_W(mr, 3, 4)
    cl = _make(mr, 4, 3)
    cl.run_decoupled(_x0(mr, 3), 2, Wr[:2])
    refused(cl, "leave no per-batch plan")
    cl.step(Wr[2], fetch=False)      # a solved step makes a plan again
    cl.hold_step(Wr[3], fetch=False)
    assert (cl.f.get("hold_index", (), np.int32) == 1).all()
    cl.close()


# ---- 7: rerun ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,B,M", [("pendulum", 4, 5, 3), ("rocket", 4, 70, 2)])
def test_second_identical_run_gives_identical_bits(model, N, B, M):
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    steps = 5
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    outs = []
    cl = _make(m, N, B, solve_every=M)
    for _ in range(2):      # the same handle twice: the second run starts from whatever the first left in the hold state and the log
        outs.append(cl.run_on_device(x0, steps, W))
        outs[-1]["final_xi"] = cl.f.get("hold_xi", (N + 1, m.nx))
    cl.close()
    cl = _make(m, N, B)
    outs.append(cl.run(x0, steps, W, solve_every=M))      # the host-fetching loop records the same run
    dec = cl.run_decoupled(x0, steps, W, solve_every=M)    # M > 1: the step-by-step loop, as for solve_waves > 1
    cl.close()
    assert dec["rounds"] == steps and "qp_stats" not in dec
    for k in outs[0]:
        if not k.startswith("t_") and k != "final_xi":
            assert np.array_equal(dec[k], outs[0][k], equal_nan=True), k
    assert outs[0]["hold_index"].any() and outs[0]["hold_policy"].any()
    for k in outs[0]:
        if not k.startswith("t_"):
            assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k
    for k in ("input_trajectory", "hold_index", "hold_policy", "success", "nominal_trajectory_u", "backoff_trajectory_x"):
        assert np.array_equal(outs[2][k], outs[0][k]), k
    hold_at = np.arange(steps) % M != 0
    assert np.array_equal(outs[2]["state_trajectory"][:, :, hold_at], outs[0]["state_trajectory"][:, :, hold_at])


def test_monte_carlo_driver_passes_solve_every_to_its_slices():
    from robust_nonlinear_mpc_amd import get_model, run_monte_carlo
    m = get_model("rocket")
    N, S, steps, M = 4, 5, 4, 2
    x0 = m.x_ref + 0.3 * (m.extra["x0"] - m.x_ref)
    r = run_monte_carlo(m, N, np.arange(S), steps, x0, slices=2, solve_every=M)
    cl = _make(m, N, S, solve_every=M)
    out = cl.run_on_device(np.tile(x0, (S, 1)), steps, _seeded_W(m, S, steps))
    cl.close()
    assert np.array_equal(r["hold_index"], np.tile(np.arange(steps) % M, (S, 1)))
    for k in ("state_trajectory", "input_trajectory", "hold_index", "hold_policy", "success"):
        assert np.array_equal(r[k], out[k]), k
    plain = run_monte_carlo(m, N, np.arange(S), steps, x0, slices=2)
    assert "hold_index" not in plain and not np.array_equal(plain["input_trajectory"], r["input_trajectory"])

"""Time-varying and per-instance box bounds in the on-device closed loops (slsqp_cl_set_bounds): against the CPU restatement of the bounded loop,
the rows of slsqp_linearize and of the tightened QP against numpy, bit for bit between the entry points (step by step, persistent, round-based), the
no-op equivalences, the hold of the last row, the stage-0 gate, +inf rows, the nominal initialiser, the refusals and the Monte-Carlo driver."""
import ctypes as C

import numpy as np
import pytest

import bounds_cases as BC
from test_gpu_reference import LOG_KEYS, _assert_same, _decoupled, _seeded_W, _stepwise, _wavy_reference

pytestmark = pytest.mark.gpu


def _make(m, N, B, rti=None, rti_steps=None, bounds=None, tune=None, **kw):
    from robust_nonlinear_mpc_amd import ClosedLoopMPC
    cl = ClosedLoopMPC(m, N, B, rti=rti, fast_sls_rti_steps=rti_steps, bounds=bounds, **kw)
    if tune:
        tune(cl.f.opts)
    return cl


def _wavy_bounds(m, B, T, amp):
    """Per-instance bounds that vary in time: every side of the model's box pulled in by up to `amp` of its value, a different amount per (instance,
    row, component); the terminal rows likewise."""
    t, b = np.arange(T)[None, :, None], np.arange(B)[:, None, None]
    def pull(base):
        i = np.arange(len(base))[None, None, :]
        return np.asarray(base, dtype=float) * (1.0 - amp * (0.5 + 0.5 * np.sin(0.35 * t + 0.7 * b + 0.3 * i)))
    return pull(m.g), pull(m.gf)


def _logged(cl, x0, steps):
    out = cl.run_on_device(x0, steps)
    cl.close()
    return out


def _rocket_start(m, B):
    return np.tile(m.x_ref + 0.3 * (m.extra["x0"] - m.x_ref), (B, 1)), dict(solve_nominal=True, continuation=2)


# ---- 1: against the CPU restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["cl_step", "cl_run_scp"])
@pytest.mark.parametrize("plant", ["P", "Q"])
def test_bounded_closed_loop_vs_oracle(plant, run):
    """The three cases of a plant as ONE per-instance batch, script settings, through slsqp_cl_step and slsqp_cl_run_scp: state, u0 and the nominal
    at the 1e-6 relative of tests/test_gpu_reference.py, success equal.  The CPU runs differ from the unbounded ones by > 1e-3
    (tests/test_bounds_cpu.py), so 1e-6 separates them."""
    names = [plant + str(i) for i in (1, 2, 3)]
    cs = [BC.case(n) for n in names]
    m, N, steps, B = cs[0]["m"], cs[0]["N"], cs[0]["steps"], 3
    bounds = (np.stack([c["g"] for c in cs]), np.stack([c["gf"] for c in cs]))
    cl = _make(m, N, B, bounds=bounds)
    x0 = np.stack([c["x0"] for c in cs])
    out = cl.run_on_device(x0, steps) if run == "cl_step" else cl.run_decoupled(x0, steps)
    cl.close()
    assert out["constraint_margin"].shape == (steps, B)
    for b, name in enumerate(names):
        ref = BC.oracle_case(name)
        assert ref["success"].all() and ref["oracle_qp_converged"].all()
        scale = max(1.0, np.abs(ref["nominal_x"]).max())
        errs = dict(
            state=np.max(np.abs(out["state_trajectory"][b].T - ref["state"])) / scale,
            u0=np.max(np.abs(out["input_trajectory"][b].T - ref["u0"][: steps - 1])) / max(1.0, np.abs(ref["u0"]).max()),
            nominal_x=np.max(np.abs(out["nominal_trajectory_x"][b].transpose(2, 1, 0) - ref["nominal_x"])) / scale,
            nominal_u=np.max(np.abs(out["nominal_trajectory_u"][b].transpose(2, 1, 0) - ref["nominal_u"])) / max(1.0, np.abs(ref["nominal_u"]).max()))
        print(name, run, errs, "constraint_margin", out["constraint_margin"][:, b].min())
        assert list(out["success"][b]) == list(ref["success"])
        for k, e in errs.items():
            assert e < 1e-6, (name, k, e)


# ---- 2: slsqp_linearize ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_instance", [True, False])
@pytest.mark.parametrize("model,N", [("pendulum", 10), ("rocket", 5)])
def test_linearize_forms_the_windowed_rows_and_nothing_else(model, N, per_instance):
    """g, gN = the window's rows -/+ the nominal as numpy forms them, to the last bit, at handle step counts 0 and T - 2 (there the hold begins inside
    the horizon); A, Bm, c, q keep the bits of a handle without bounds."""
    from robust_nonlinear_mpc_amd import BatchedFastSLS, get_model
    m = get_model(model)
    B, T = 3, 4
    nx, nz = m.nx, m.nz
    rng = np.random.default_rng(7)
    X = m.x_ref + 0.05 * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, (B, N + 1, nx))
    U = m.u_ref + 0.05 * (m.u_ub - m.u_lb) * rng.uniform(-1, 1, (B, N, m.nu))
    g, gf = _wavy_bounds(m, B, T, 0.3)
    if not per_instance:
        g, gf = g[1], gf[1]
    shapes = dict(A=(N, nx, nx), Bm=(N, nx, m.nu), c=(N, nx), g=(N, m.ni), gN=(m.ni_f,), q=(m.n_var(N),))
    f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=B)
    f.linearize(X, U)
    plain = {k: f.get(k, s) for k, s in shapes.items()}
    f.close()
    cl = _make(m, N, B, bounds=(g, gf))
    cl.reset(np.tile(m.x_ref, (B, 1)) if model == "rocket" else np.tile(m.extra["x0"], (B, 1)))
    for s in (0, T - 2):
        while cl.steps_done < s:
            cl.step(None, fetch=False)
        cl.f.linearize(X, U)
        got = {k: cl.f.get(k, sh) for k, sh in shapes.items()}
        for b in range(B):
            gw, gfw = BC.bounds_window(g[b] if per_instance else g, gf[b] if per_instance else gf, s, N)
            z = np.concatenate([X[b, :N], U[b]], axis=1)
            assert np.array_equal(got["g"][b], np.concatenate([gw[:, :nz] - z, gw[:, nz:] + z], axis=1)), (s, b)
            assert np.array_equal(got["gN"][b], np.concatenate([gfw[:nx] - X[b, N], gfw[nx:] + X[b, N]])), (s, b)
        assert not np.array_equal(got["g"], plain["g"]) and not np.array_equal(got["gN"], plain["gN"])
        for k in ("A", "Bm", "c", "q"):
            assert np.array_equal(got[k], plain[k]), (s, k)
    cl.close()


# ---- 3: tightened rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [1, 2])
def test_tightened_rows_use_the_window(fuse):
    """After one slsqp_cl_step at MPC step s = 2 (rti 1, one fast-SLS step; fuse 1: the separate launches with k_tighten, 2: the fused chain): the
    terminal rows of ubg are gf_row(min(s + N, T - 1)) - backoff_f, un-shifted, and the stage rows g_k - backoff_k, with the device's own operands.
    Every instance's terminal row differs from the model's gf.  conv_tol = 0: the fast-SLS convergence check against the previous MPC step's solution
    (quirk q5) would otherwise skip the sweep and the tightening at this step, and ubg would hold the un-tightened rows."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, T, s = 10, 3, 14, 2
    nx, ni, nif = m.nx, m.ni, m.ni_f
    g, gf = _wavy_bounds(m, B, T, 0.2)

    def tune(o):
        o.fuse_rti, o.conv_tol = fuse, 0.0
    cl = _make(m, N, B, 1, 1, (g, gf), tune)
    cl.reset(np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.1 * np.arange(B)[:, None]))
    for _ in range(s + 1):
        cl.step(None, fetch=False)
    f = cl.f
    ubg, bo, bof, c, gk = f.get("ubg", (f.mb,)), f.get("backoff", (N, ni)), f.get("backoff_f", (nif,)), f.get("c", (N, nx)), f.get("g", (N, ni))
    ok = f.get("success", (), np.int32)
    cl.close()
    assert ok.all()
    st = ubg[:, : N * (nx + ni)].reshape(B, N, nx + ni)
    for b in range(B):
        row = gf[b, min(s + N, T - 1)]
        assert not np.array_equal(row, m.gf)
        assert np.array_equal(ubg[b, N * (nx + ni):], row - bof[b]), b
        assert not np.array_equal(ubg[b, N * (nx + ni):], m.gf - bof[b])
        assert np.array_equal(st[b, :, nx:], gk[b] - bo[b]), b
        assert np.array_equal(st[b, :, :nx], -c[b]), b


# ---- 4: the loops under per-instance time-varying bounds, bit for bit the step-by-step loop ----------------------------------------------------
def _tune_converge(o):
    o.scp_eps = 1e-8


@pytest.mark.parametrize("model,N,B,steps,waves,rti,rti_steps,tune", [
    ("rocket", 20, 96, 5, 7, 1, 1, None),
    ("pendulum", 10, 50, 8, 7, 3, 2, None),
    ("pendulum", 10, 8, 2, None, -1, 2, _tune_converge),
])
def test_persistent_loops_are_bitwise_the_step_by_step_loop_with_bounds(model, N, B, steps, waves, rti, rti_steps, tune):
    """Inside the persistent launches every instance is at its own MPC step (7 waves for 96 or 50 instances: they are at different steps at the same
    time and change hands), so the window must come from the instance's own step count, in the linearisation and in the tightening.  The bounds are
    shorter than the run (T < steps + N): the hold is part of every window near the end.  Rocket: k_cl_loop, and the round-based loop; pendulum: the
    script setting and SCP converge mode (k_cl_loop_scp)."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    bounds = _wavy_bounds(m, B, steps + 4, 0.05)
    if model == "rocket":
        x0, kw = _rocket_start(m, B)
    else:
        x0, kw = np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.2 * np.random.default_rng(3).uniform(-1, 1, (B, 1))), {}
    W = _seeded_W(m, B, steps)
    ref, ref_fin = _stepwise(_make(m, N, B, rti, rti_steps, bounds, tune), steps, x0, W, **kw)
    print("success rate", ref["success"].mean())
    assert ref["success"].any()
    out, fin = _decoupled(_make(m, N, B, rti, rti_steps, bounds, tune), steps, x0, W, waves=waves, **kw)
    _assert_same(out, fin, ref, ref_fin, "persistent")
    assert out["loop_stats"]["waves"] == (B if waves is None else waves)
    assert np.array_equal(out["constraint_margin"], ref["constraint_margin"])
    if model == "rocket":
        def rounds(o):
            o.cl_persistent = 0
        out, fin = _decoupled(_make(m, N, B, rti, rti_steps, bounds, rounds), steps - 1, x0, W[: steps - 1], **kw)
        ref4, ref4_fin = _stepwise(_make(m, N, B, rti, rti_steps, bounds, tune), steps - 1, x0, W[: steps - 1], **kw)
        _assert_same(out, fin, ref4, ref4_fin, "rounds")


def test_bounds_compose_with_a_reference_and_plant_parameters():
    """One run with all three per-handle options set (rocket, 96 instances on 7 waves, 3 steps): the persistent launch against one slsqp_cl_step per
    step, every result array, qp_stats and the model error."""
    from robust_nonlinear_mpc_amd import get_model, plant_param_defaults
    m = get_model("rocket")
    N, B, steps = 20, 96, 3
    bounds = _wavy_bounds(m, B, steps + 4, 0.05)
    reference = _wavy_reference(m, B, steps + 4, 0.2)
    P = np.tile(plant_param_defaults(m), (B, 1)) * (1.0 + 0.05 * np.sin(np.arange(B))[:, None])
    x0, kw = _rocket_start(m, B)
    W = _seeded_W(m, B, steps)
    mk = lambda: _make(m, N, B, 1, 1, bounds, None, reference=reference, plant_params=P)
    ref, ref_fin = _stepwise(mk(), steps, x0, W, **kw)
    out, fin = _decoupled(mk(), steps, x0, W, waves=7, **kw)
    assert ref["success"].any()
    _assert_same(out, fin, ref, ref_fin, "persistent, all three")
    assert np.array_equal(out["model_error"], ref["model_error"]) and np.abs(out["model_error"]).max() > 0


# ---- 5: no-op equivalences ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["pendulum", "rocket"])
def test_the_models_box_set_explicitly_is_the_same_bits_as_no_bounds(model):
    """No bounds == the model's box as T = 1 shared rows == the same per instance == T = 4 equal rows == bounds set and cleared: every result array,
    qp_stats and the final state, step by step and through the persistent launch."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    if model == "pendulum":
        N, B, steps, rti, rti_steps = 10, 64, 6, None, None
        x0, W, kw = np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.2 * np.random.default_rng(3).uniform(-1, 1, (B, 1))), None, {}
    else:
        N, B, steps, rti, rti_steps = 20, 32, 3, 1, 1
        (x0, kw), W = _rocket_start(m, B), _seeded_W(m, B, steps)

    def handle(kind):
        cl = _make(m, N, B, rti, rti_steps)
        if kind == "shared":
            cl.set_bounds(m.g[None, :], m.gf[None, :])
        elif kind == "per instance":
            cl.set_bounds(np.tile(m.g, (B, 1, 1)))
        elif kind == "four rows":
            cl.set_bounds(np.tile(m.g, (4, 1)), np.tile(m.gf, (4, 1)))
        elif kind == "cleared":
            cl.set_bounds(*_wavy_bounds(m, B, 5, 0.05))
            cl.set_bounds(None)
        return cl
    for run in (_stepwise, _decoupled):
        ref, ref_fin = run(handle("never"), steps, x0, W, **kw)
        assert ref["success"].any() and "constraint_margin" not in ref
        for kind in ("shared", "per instance", "four rows", "cleared"):
            out, fin = run(handle(kind), steps, x0, W, **kw)
            _assert_same(out, fin, ref, ref_fin, (run.__name__, kind))
            assert ("constraint_margin" in out) == (kind != "cleared")


# ---- 6: the hold ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [_stepwise, _decoupled])
def test_one_row_equals_the_row_repeated(run):
    """T = 1 per-instance rows against the same rows repeated steps + N + 1 times: the same bits."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, steps = 10, 3, 5
    x0 = np.tile(m.extra["x0"], (B, 1))
    g, gf = _wavy_bounds(m, B, 1, 0.3)
    Tfull = steps + N + 1
    ref, ref_fin = run(_make(m, N, B, bounds=(g, gf)), steps, x0)
    out, fin = run(_make(m, N, B, bounds=(np.repeat(g, Tfull, axis=1), np.repeat(gf, Tfull, axis=1))), steps, x0)
    assert ref["success"].any()
    _assert_same(out, fin, ref, ref_fin, run.__name__)


# ---- 7: the stage-0 gate ---------------------------------------------------------------------------------------------------------------------------
def test_stage0_gate_reads_the_rows_of_the_steps_own_window():
    """Four instances; before MPC step 2, instance 1 gets rows whose row 2 puts the upper bound of its cart position 1e-3 below its measured state
    (rows 0, 1 and 3 are the model's box, so only stage 0 of step 2 sees it).  That instance's first QP is refused with status 2 and x0_viol equal to
    the excess over the row as the QP holds it (every bound row of the QP carries k_set_bounds' pad of 1e-10, and the gate measures against that
    row); the other three keep the bits of a run without it.  With x0_box_tol = 1e-2 the step is accepted.  A refused QP is an ordinary status."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B = 10, 4
    x0 = np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.1 * np.arange(B)[:, None])

    def run(exclude, tol=0.0):
        cl = _make(m, N, B, 1, 1, x0_box_tol=tol, bounds=(m.g[None, :], m.gf[None, :]))      # (one SCP iteration: the step's qp_stats are those of its only solve)
        cl.reset(x0)
        cl.step(None, fetch=False)
        r = cl.step(None)
        xm = r["x_next"]
        excess = None
        if exclude:
            g = np.tile(m.g, (B, 4, 1))
            g[1, 2, 0] = xm[1, 0] - 1e-3
            excess = xm[1, 0] - (g[1, 2, 0] + 1e-10)
            cl.set_bounds(g)
        r = cl.step(None)
        r["qp_status"] = cl.f.get("qp_stats", (2, 8), np.int32)[:, :, 6]
        cl.close()
        return r, excess
    ref, _ = run(False)
    out, excess = run(True)
    assert ref["success"].all()
    assert out["qp_status"][1, 0] == 2 and not out["success"][1]
    print("excess", excess, "x0_violation", out["x0_violation"][1])
    assert abs(out["x0_violation"][1, 0] - excess) < 1e-12 and abs(excess - 1e-3) < 1e-9
    others = [0, 2, 3]
    for k in ("u0", "x_next", "nominal_x", "nominal_u", "backoff_x", "backoff_u", "success", "status", "x0_violation"):
        assert np.array_equal(out[k][others], ref[k][others]), k
    acc, _ = run(True, tol=1e-2)
    assert acc["success"].all() and acc["qp_status"][1, 0] == 0
    assert abs(acc["x0_violation"][1, 0] - excess) < 1e-12


# ---- 8: +inf rows ----------------------------------------------------------------------------------------------------------------------------------
def test_infinite_rows_are_no_bound():
    """Both sides of a never-active component (the pendulum's angular velocity) at +inf: same success, trajectories within 1e-9 of the model's box.
    One side of the ACTIVE input bound of case P1 at +inf frees it.  The bound is active through its tightened row (0.22 minus the tube's back-off)
    on the side the predicted inputs of MPC times 3 .. lean to; with that side at +inf the predictions go as far out as the unbounded loop's, more
    than 1e-2 beyond the bounded loop's, and constraint_margin does not hold the input against the infinite row."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    c = BC.case("P1")
    N, steps, nx, nz = c["N"], c["steps"], m.nx, m.nz
    x0 = c["x0"][None, :]
    plain = _logged(_make(m, N, 1), x0, steps)
    g = np.tile(m.g, (1, 1)); g[0, 3] = np.inf; g[0, nz + 3] = np.inf
    gf = np.tile(m.gf, (1, 1)); gf[0, 3] = np.inf; gf[0, nx + 3] = np.inf
    free = _logged(_make(m, N, 1, bounds=(g, gf)), x0, steps)
    assert np.array_equal(free["success"], plain["success"]) and plain["success"].all()
    for k in ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u"):
        assert np.max(np.abs(free[k] - plain[k])) < 1e-9, k
    assert np.isfinite(free["constraint_margin"]).all()
    k, t = np.meshgrid(np.arange(N), np.arange(steps), indexing="ij")
    pred = lambda o: o["nominal_trajectory_u"][0, 0][k + t >= 3]      # every step's predicted inputs of MPC times 3 ..
    upper = pred(plain).max() > -pred(plain).min()
    far = (lambda o: pred(o).max()) if upper else (lambda o: -pred(o).min())      # how far out on the side the predictions lean to
    held = _logged(_make(m, N, 1, bounds=(c["g"], c["gf"])), x0, steps)
    g1 = c["g"].copy(); g1[:, nx if upper else nz + nx] = np.inf
    out = _logged(_make(m, N, 1, bounds=(g1, c["gf"])), x0, steps)
    print("upper side" if upper else "lower side", "unbounded", far(plain), "bounded", far(held), "that side freed", far(out))
    assert held["success"].all() and out["success"].all()
    assert far(held) <= 0.22 and far(plain) > far(held) + 1e-2
    assert far(out) > far(held) + 1e-2 and abs(far(out) - far(plain)) < 1e-3
    assert np.isfinite(out["constraint_margin"]).all() and out["constraint_margin"].min() >= -1e-9


# ---- 9: the initialiser ----------------------------------------------------------------------------------------------------------------------------
def test_nominal_initialiser_respects_the_window_of_step_0():
    """reset(solve_nominal=True) on the rocket with a per-instance bound on the thrust command at 95 % of the peak of the unbounded first nominal (on
    the side where that nominal peaks): the bounded nominal satisfies its own box to 1e-8 and the dynamics to the 1e-6 of tests/test_gpu_reference.py; the unbounded one violates
    that box."""
    from problems import host_ddyn
    from robust_nonlinear_mpc_amd import box_bounds, get_model
    m = get_model("rocket")
    N, B = 20, 3
    nx, nz = m.nx, m.nz
    x0 = np.stack([m.x_ref + s * (m.extra["x0"] - m.x_ref) for s in (0.2, 0.25, 0.3)])

    def nominal(bounds):
        cl = _make(m, N, B, 1, 1, bounds)
        cl.reset(x0, solve_nominal=True, continuation=2)
        X, U, st = cl.f.get("nominal_x", (N + 1, nx)), cl.f.get("nominal_u", (N, m.nu)), cl.nlp_status
        cl.close()
        return X, U, st
    X0, U0, st0 = nominal(None)
    up = U0[:, :, 0].max(axis=1) >= (-U0[:, :, 0]).max(axis=1)
    peak = np.where(up, U0[:, :, 0].max(axis=1), (-U0[:, :, 0]).max(axis=1))
    print("nlp_status", st0, "peak", peak, "upper side", up)
    assert (st0 == 0).all() and (peak > 1e-2).all(), (st0, peak)
    T = N + 1
    side = lambda on: np.tile(np.where(on, 0.95 * peak, np.inf)[:, None], (1, T))
    g, gf = box_bounds(m, T, {nx: (-side(~up), side(up))}, batch=B)
    X, U, st = nominal((g, gf))
    print("nlp_status", st, "bounded extremes", U[:, :, 0].max(axis=1), U[:, :, 0].min(axis=1))
    for b in range(B):
        gw, gfw = BC.bounds_window(g[b], gf[b], 0, N)
        def viol(Xb, Ub):
            zz = np.concatenate([Xb[:N], Ub], axis=1)
            v = np.concatenate([zz - gw[:, :nz], -zz - gw[:, nz:]], axis=1)
            v[0, :nx] = -np.inf; v[0, nz:nz + nx] = -np.inf      # x_0 is data
            return max(v.max(), (Xb[N] - gfw[:nx]).max(), (-Xb[N] - gfw[nx:]).max())
        defect = max(np.abs(X[b, 0] - x0[b]).max(), max(np.abs(host_ddyn(m.model_id, X[b, k], U[b, k]) - X[b, k + 1]).max() for k in range(N)))
        assert defect < 1e-6 and viol(X[b], U[b]) < 1e-8, (b, defect, viol(X[b], U[b]))
        assert viol(X0[b], U0[b]) > 1e-4, (b, viol(X0[b], U0[b]))


# ---- 10: refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_leave_the_bounds_in_force():
    from robust_nonlinear_mpc_amd import BatchedFastSLS, get_model
    L = __import__("robust_nonlinear_mpc_amd")._lib
    m = get_model("pendulum")
    N, B, T = 10, 2, 4
    nz = m.nz
    f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=B)
    rng = np.random.default_rng(1)
    X, U = 0.1 * rng.uniform(-1, 1, (B, N + 1, m.nx)), 0.1 * rng.uniform(-1, 1, (B, N, m.nu))
    assert np.array_equal(f.get("bounds_g", (1, m.ni)), np.tile(m.g, (B, 1, 1))) and np.array_equal(f.get("bounds_gf", (1, m.ni_f)), np.tile(m.gf, (B, 1, 1)))
    g, gf = _wavy_bounds(m, B, T, 0.2)
    f.set_bounds(g, gf)
    assert np.array_equal(f.get("bounds_g", (T, m.ni)), g) and np.array_equal(f.get("bounds_gf", (T, m.ni_f)), gf)

    def rows_now():
        f.linearize(X, U)
        return f.get("g", (N, m.ni)), f.get("gN", (m.ni_f,))
    ref = rows_now()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    def spoil(a, idx, v):
        a = a.copy(); a[idx] = v
        return a
    cross = g.copy(); cross[1, 2, 1] = -cross[1, 2, nz + 1] - 1e-6
    crossf = gf.copy(); crossf[0, 0, 0] = -crossf[0, 0, m.nx] - 1e-6
    keep = [spoil(g, (1, 2, 0), np.nan), spoil(gf, (0, 1, 3), np.nan), spoil(g, (0, 0, 2), -np.inf), cross, crossf]
    for args, word in (((ptr(g), ptr(gf), -1, 1), "T"), ((ptr(g), ptr(gf), 0, 1), "T = 0"), ((None, None, T, 1), "NULL"), ((None, ptr(gf), T, 0), "NULL"),
                       ((ptr(g), ptr(gf), T, 2), "per_instance"), ((ptr(g), ptr(gf), T, -1), "per_instance"),
                       ((ptr(keep[0]), ptr(gf), T, 1), "NaN"), ((ptr(g), ptr(keep[1]), T, 1), "NaN"), ((ptr(keep[2]), ptr(gf), T, 1), "-inf"),
                       ((ptr(keep[3]), ptr(gf), T, 1), "below"), ((ptr(g), ptr(keep[4]), T, 1), "below")):
        assert f.lib.slsqp_cl_set_bounds(f.h, *args, L.HOST) < 0, (args, word)
        assert word in f.lib.slsqp_last_error().decode(), (word, f.lib.slsqp_last_error().decode())
        now = rows_now()
        assert np.array_equal(now[0], ref[0]) and np.array_equal(now[1], ref[1]), word
    for bad in (lambda: f.set_bounds(np.tile(m.g, (B + 1, T, 1))), lambda: f.set_bounds(g, gf[:, :-1]), lambda: f.set_bounds(keep[0], gf), lambda: f.set_bounds(cross),
                lambda: f.set_bounds(None, gf)):
        with pytest.raises(ValueError):
            bad()
    now = rows_now()
    assert np.array_equal(now[0], ref[0]) and np.array_equal(now[1], ref[1])
    assert np.array_equal(f.get("bounds_g", (T, m.ni)), g)
    # +inf is accepted; shared rows with gf = NULL repeat the model's gf; then cleared
    f.set_bounds(spoil(g[0], (1, 0), np.inf))
    assert np.isinf(f.get("bounds_g", (T, m.ni))[1, 1, 0]) and np.array_equal(f.get("bounds_gf", (T, m.ni_f)), np.tile(m.gf, (B, T, 1)))
    f.set_bounds(None)
    assert np.array_equal(f.get("bounds_g", (1, m.ni)), np.tile(m.g, (B, 1, 1)))
    z = np.concatenate([X[:, :N], U], axis=2)
    assert np.array_equal(rows_now()[0], np.concatenate([m.g[:nz] - z, m.g[nz:] + z], axis=2))
    # loc outside {host, device}; then a handle whose constraints were replaced by a general G (the sweep-level boundary's): both refused, and the
    # bounds set before stay what slsqp_get reports
    f.set_bounds(g, gf)
    assert f.lib.slsqp_cl_set_bounds(f.h, ptr(g), ptr(gf), T, 1, 7) < 0 and "loc" in f.lib.slsqp_last_error().decode()
    now = rows_now()
    assert np.array_equal(now[0], ref[0]) and np.array_equal(now[1], ref[1])
    G = np.ascontiguousarray(m.G, dtype=float).copy(); G[0, 1] = 0.5
    Gf, gfm = np.ascontiguousarray(m.Gf, dtype=float), np.ascontiguousarray(m.gf, dtype=float)
    L.check(f.lib.slsqp_set_constraints(f.h, ptr(G), ptr(Gf), ptr(gfm)))
    smaller = 0.5 * g
    assert f.lib.slsqp_cl_set_bounds(f.h, ptr(smaller), ptr(gf), T, 1, L.HOST) < 0 and "general G" in f.lib.slsqp_last_error().decode()
    assert f.lib.slsqp_cl_set_bounds(f.h, None, None, 0, 0, L.HOST) < 0 and "general G" in f.lib.slsqp_last_error().decode()
    with pytest.raises(RuntimeError, match="general G"):
        f.set_bounds(smaller, gf)
    assert np.array_equal(f.get("bounds_g", (T, m.ni)), g) and np.array_equal(f.get("bounds_gf", (T, m.ni_f)), gf)
    assert f.bounds is not None and np.array_equal(f.bounds[0], g)
    G = np.ascontiguousarray(m.G, dtype=float)
    L.check(f.lib.slsqp_set_constraints(f.h, ptr(G), ptr(Gf), ptr(gfm)))      # the box again: the previous bounds are still the ones in force
    now = rows_now()
    assert np.array_equal(now[0], ref[0]) and np.array_equal(now[1], ref[1])
    f.close()
    # a handle without a plant model is refused
    from robust_nonlinear_mpc_amd.fast_sls import _ModelView
    mv = _ModelView(m); mv.model_id = None
    f = BatchedFastSLS(N, m.Q, m.R, mv, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=B)
    assert f.lib.slsqp_cl_set_bounds(f.h, ptr(g), ptr(gf), T, 1, L.HOST) < 0 and "slsqp_set_model" in f.lib.slsqp_last_error().decode()
    f.close()


# ---- 11: Monte-Carlo driver ----------------------------------------------------------------------------------------------------------------------------
def test_monte_carlo_cuts_per_seed_bounds_with_the_seeds(tmp_path):
    """run_monte_carlo(bounds=per seed) in one slice and cut into two gives the same rows; constraint_margin is part of the result and of the npz."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model, run_monte_carlo
    m = get_model("quadrotor")
    N, S, steps = 10, 5, 3
    x0 = m.x_ref + 0.02 * (m.x_ub - m.x_lb)
    x0[6:10] /= np.linalg.norm(x0[6:10])
    bounds = _wavy_bounds(m, S, steps + 3, 0.05)
    kw = dict(noise=True, gather=False)
    one = run_monte_carlo(m, N, np.arange(S), steps, x0, bounds=bounds, **kw)
    two = run_monte_carlo(m, N, np.arange(S), steps, x0, bounds=bounds, slices=2, **kw)
    plain = run_monte_carlo(m, N, np.arange(S), steps, x0, **kw)
    assert one["success"].any()
    for k in LOG_KEYS + ("constraint_margin", "bounds_g", "bounds_gf"):
        assert np.array_equal(one[k], two[k], equal_nan=True), k
    assert one["constraint_margin"].shape == (steps, S) and np.array_equal(one["bounds_g"], bounds[0])
    assert "constraint_margin" not in plain
    cl = ClosedLoopMPC(m, N, S)
    cl.save_npz(str(tmp_path / "b.npz"), one, 2)
    cl.save_npz(str(tmp_path / "p.npz"), plain, 2)
    cl.close()
    kb, kp = set(np.load(tmp_path / "b.npz").files), set(np.load(tmp_path / "p.npz").files)
    assert kb - kp == {"constraint_margin", "bounds_g", "bounds_gf"} and kp <= kb
    zb = np.load(tmp_path / "b.npz")
    assert np.array_equal(zb["bounds_g"], bounds[0][2]) and np.array_equal(zb["constraint_margin"], one["constraint_margin"][:, 2])

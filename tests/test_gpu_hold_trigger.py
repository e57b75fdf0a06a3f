"""Event-triggered solves in the persistent closed-loop launch (slsqp_cl_set_hold_trigger, slsqp_cl_tube_ratio).

An instance holds its plan while its measured state stays inside theta x the tube that plan computed and solves when it does not, or after M steps.
The comparisons: the logged schedule against tests/hold_trigger_ref.py (numpy) recomputed from the result's own arrays; every instance's run against
a replay of ITS schedule on a fresh handle with step() / hold_step(), np.array_equal (instances of a batch do not influence one another:
tests/test_gpu_hold.py, tests/test_gpu_hold_persistent.py); theta = inf against the fixed period and theta = 0 against M = 1, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import bounds_cases as BC
import hold_trigger_ref as T
import plant_params_helpers as H
import reference_cases as RC

pytestmark = pytest.mark.gpu

INF = float("inf")
RTOL = 4e-16      # one subtraction and one division, both correctly rounded; the build has no fast-math
# Amplitudes max_i |w_i| of the plant's disturbance samples.  Near the neutral point the ratio of a first hold step is 0.50 to 0.72 of the amplitude on
# all three models (measured: DESIGN.md section 21), so LO puts a first hold step at 0.05 .. 0.07 of its
# tube and HI at 0.9 .. 1.3: both well outside [theta / 1.5, 1.5 theta] for theta = 0.5.  (HI is outside the unit box the tubes assume: that is how a
# state leaves its tube.)
LO, HI = 0.1, 1.8


def _lib():
    return __import__("robust_nonlinear_mpc_amd")._lib


def _make(m, N, B, rti=1, rti_steps=1, **kw):
    from robust_nonlinear_mpc_amd import ClosedLoopMPC
    return ClosedLoopMPC(m, N, B, rti=rti, fast_sls_rti_steps=rti_steps, **kw)


def _x0(m, B, scale=0.3):
    """Per-instance initial states, as tests/test_gpu_hold_persistent.py."""
    rng = np.random.default_rng(21)
    if m.name == "quadrotor":
        x0 = m.x_ref + 0.02 * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, (B, m.nx))
        x0[:, 6:10] /= np.linalg.norm(x0[:, 6:10], axis=1, keepdims=True)
        return x0
    s = scale if m.name == "rocket" else 1.0
    return m.x_ref + s * (m.extra["x0"] - m.x_ref) * (1.0 + 0.1 * rng.uniform(-1, 1, (B, 1)))


def _x0_near(m, B):
    """The same states pulled towards the neutral point until the plan's dynamics defect is small against E (the rocket's E is 8.7e-5 in qw): the
    ratio of a first hold step is then max_i |w_i| to a few per cent."""
    if m.name == "quadrotor":
        rng = np.random.default_rng(21)
        x0 = m.x_ref + NEAR[m.name] * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, (B, m.nx))
        x0[:, 6:10] /= np.linalg.norm(x0[:, 6:10], axis=1, keepdims=True)
        return x0
    return m.x_ref + NEAR[m.name] * (_x0(m, B, 1.0) - m.x_ref)


NEAR = {"rocket": 0.01, "pendulum": 0.02, "quadrotor": 0.0005}


def _seeded_W(m, B, steps):
    from robust_nonlinear_mpc_amd import disturbance_stream
    return np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)


def _amplitudes(B, steps, M):
    """(steps, B) in {LO, HI}: instance b's first b % steps plant steps are large.  Each of them follows a solve and makes the next step a solve
    (reason 2, at k = 1 < M); from then on the instance is well inside its tube and holds M - 1 steps in a row.  Instance 0 never leaves half its
    tube.  `steps` different schedules in a batch of that many instances."""
    amp = np.full((steps, B), LO)
    for b in range(B):
        amp[:b % steps, b] = HI
    return amp


def _scaled_W(m, B, steps, M):
    """The seeded stream scaled per instance and step so that max_i |w_i| is the amplitude."""
    W = _seeded_W(m, B, steps)
    return W * (_amplitudes(B, steps, M) / np.abs(W).max(axis=2))[:, :, None]


def _final(cl):
    m, N, f = cl.m, cl.N, cl.f
    return dict(x_meas=f.get("x_meas", (m.nx,)), nominal_x=f.get("nominal_x", (N + 1, m.nx)), nominal_u=f.get("nominal_u", (N, m.nu)), u0=f.get("u0", (m.nu,)),
                hold_xi=f.get("hold_xi", (N + 1, m.nx)), hold_index=f.get("hold_index", (), np.int32), hold_policy=f.get("hold_policy", (), np.int32))


def _same(a, b, skip=(), row=None):
    """Every shared key but the timings; row = b: instance b's part of every per-instance array alone."""
    shared = [k for k in a if k in b and not k.startswith("t_") and k not in skip]
    assert shared
    for k in shared:
        x, y = a[k], b[k]
        if row is not None and k in ("disturbance_used", "constraint_margin"):      # (steps, B)
            x, y = x[:, row], y[:, row]
        elif row is not None and k not in ("plant_params", "bounds_g", "bounds_gf"):      # (as given, the same in both)
            x, y = x[row], y[row]
        assert np.array_equal(x, y, equal_nan=True), k


def _same_rerun(a, b):
    """tests/test_gpu_hold_persistent.py's rule for a second run on a used handle: step 0's qp_stats in their status only."""
    _same(a, b, skip=("loop_stats", "qp_stats"))
    assert np.array_equal(a["qp_stats"][:, 1:], b["qp_stats"][:, 1:]) and np.array_equal(a["qp_stats"][:, 0, :, 6], b["qp_stats"][:, 0, :, 6])


def _triggered(m, N, B, M, steps, x0, W, theta, waves=None, cl=None, **kw):
    """The persistent launch with event-triggered solves: result, final state (the handle is closed unless it was passed in)."""
    own = cl is None
    if own:
        cl = _make(m, N, B, **kw)
    if waves is not None:
        os.environ["SLSQP_LOOP_WAVES"] = str(waves)
    try:
        out = cl.run_decoupled(x0, steps, W, solve_every=M, persistent_hold=True, hold_trigger=theta)
    finally:
        os.environ.pop("SLSQP_LOOP_WAVES", None)
    assert cl.f.get_hold_trigger() == INF and cl.f.get_solve_every() == 1      # the handle's theta and M were that call's
    fin = _final(cl)
    if own:
        cl.close()
    return out, fin


def _decision(cl, b, s, k_prev, M, theta):
    """What the helper decides for instance b's step s from what the handle holds now: (code, ratio)."""
    if s == 0:
        return T.SCHEDULED, 0.0
    m, N, f = cl.m, cl.N, cl.f
    ok = bool(f.get("scp_success", (), np.int32)[b])
    r = 0.0
    if ok:
        r = float(T.tube_ratio(f.get("x_meas", (m.nx,))[b], f.get("nominal_x", (N + 1, m.nx))[b, 1], f.get("backoff_x", (N + 1, m.nx))[b, k_prev + 1]))
    return T.decide(s, k_prev, M, ok, r, theta), r


def _replay(m, N, B, M, steps, x0, W, theta, out, b, **kw):
    """Instance b's schedule of the triggered run `out`, replayed for the whole batch on a fresh handle with step() / hold_step(); at every step the
    helper's decision from the handle's own x_meas, nominal_x, backoff_x, scp_success is the schedule's.  Result, final state."""
    cl = _make(m, N, B, **kw)
    _lib().check(cl.f.lib.slsqp_cl_log(cl.f.h, steps))
    cl.reset(x0)
    k_prev = 0
    for s in range(steps):
        code, r = _decision(cl, b, s, k_prev, M, theta)
        assert code == out["solve_trigger"][b, s] and np.isclose(r, out["tube_ratio"][b, s], rtol=RTOL, atol=0), (b, s, code, r)
        if code == T.HOLD:
            assert np.isclose(cl.tube_ratio()[b], r, rtol=RTOL, atol=0)      # slsqp_cl_tube_ratio: the same number
            cl.hold_step(W[s], fetch=False)
            k_prev += 1
        else:
            cl.step(W[s], fetch=False)
            k_prev = 0
        assert k_prev == out["hold_index"][b, s]
    z = np.zeros((steps, 1))
    rep = cl._log_result(steps, z, z, z)
    rep.update(hold_index=cl.f.get("log_hold", (steps,), np.int32), hold_policy=cl.f.get("log_hold_policy", (steps,), np.int32).astype(bool))
    fin = _final(cl)
    cl.close()
    return rep, fin


def _check_schedule(out, M, theta):
    """4a: the helper reproduces the logged schedule from the result's own arrays."""
    ratio, reason, hold = T.schedule_from_log(out, M, theta)
    assert np.array_equal(reason, out["solve_trigger"]) and np.array_equal(hold, out["hold_index"])
    np.testing.assert_allclose(out["tube_ratio"], ratio, rtol=RTOL, atol=0)


def _check_replays(m, N, B, M, steps, x0, W, theta, out, fin, which, **kw):
    """4b: every instance of `which` against the stepped replay of its own schedule."""
    for b in which:
        rep, rep_fin = _replay(m, N, B, M, steps, x0, W, theta, out, b, **kw)
        _same(out, rep, row=b)
        _same(fin, rep_fin, row=b)
        assert set(fin) == set(rep_fin)


def _check_qp_stats(out, B, steps):
    """4c: "took no part" exactly at the held steps."""
    held = out["hold_index"] != 0
    qs = out["qp_stats"]
    assert qs.shape == (B, steps, 2, 8) and out["loop_stats"]["mpc_steps"] == B * steps and out["rounds"] == 1
    assert (qs[held][..., 6] == -1).all() and not np.delete(qs[held], 6, axis=-1).any()
    assert (qs[~held][:, 0, 6] != -1).all()      # a solved step ran its first QP
    assert np.array_equal(held, out["solve_trigger"] == T.HOLD)
    assert not out["x0_violation"][held].any() and not out["scp_iterations"][held].any()


def _check_conditions(out, M, theta):
    """What the inputs were chosen for: no decision hangs on rounding, a tube trigger before the cap, and a full run of holds."""
    trig, hold, r = out["solve_trigger"], out["hold_index"], out["tube_ratio"]
    evaluated = np.zeros_like(trig, dtype=bool)
    evaluated[:, 1:] = out["success"][:, :-1]
    assert evaluated.any() and not ((r[evaluated] >= theta / 1.5) & (r[evaluated] <= 1.5 * theta)).any(), r
    prev = np.concatenate([np.zeros_like(hold[:, :1]), hold[:, :-1]], axis=1)
    assert ((trig == T.TUBE) & (prev + 1 < M)).any()
    assert (hold == M - 1).any()
    assert (trig[:, 0] == T.SCHEDULED).all() and not r[:, 0].any()


# ---- 1: slsqp_cl_tube_ratio ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,B", [("rocket", 4, 3), ("pendulum", 4, 5), ("quadrotor", 3, 3)])
def test_tube_ratio_is_the_numpy_ratio_and_changes_nothing(model, N, B):
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    M, steps = 3, 6
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    a = _make(m, N, B)
    plain = a.run_on_device(x0, steps, W, solve_every=M)
    plain_fin = _final(a)
    a.close()
    cl = _make(m, N, B)
    _lib().check(cl.f.lib.slsqp_cl_log(cl.f.h, steps))
    cl.reset(x0)
    with pytest.raises(RuntimeError, match="slsqp_cl_tube_ratio: no slsqp_cl_step since slsqp_cl_init"):
        cl.tube_ratio()
    seen = []
    for s in range(steps):
        if s > 0:
            k = s % M if s % M else M      # the hold step that would come next, whether or not the loop takes it
            if k <= N - 1:
                r = cl.tube_ratio()
                ok = cl.f.get("scp_success", (), np.int32).astype(bool)
                ref = T.tube_ratio(cl.f.get("x_meas", (m.nx,)), cl.f.get("nominal_x", (N + 1, m.nx))[:, 1], cl.f.get("backoff_x", (N + 1, m.nx))[:, k])
                np.testing.assert_allclose(r[ok], ref[ok], rtol=RTOL, atol=0)
                assert np.isposinf(r[~ok]).all() and ok.any() and (r[ok] > 0).all()
                seen.append(k)
            else:
                with pytest.raises(RuntimeError, match="at most N - 1 hold steps"):
                    cl.tube_ratio()
        if s % M:
            cl.hold_step(W[s], fetch=False)
        else:
            cl.step(W[s], fetch=False)
    assert 1 in seen and 2 in seen
    z = np.zeros((steps, 1))
    out = cl._log_result(steps, z, z, z)
    out.update(hold_index=cl.f.get("log_hold", (steps,), np.int32), hold_policy=cl.f.get("log_hold_policy", (steps,), np.int32).astype(bool))
    _same(out, plain)
    _same(_final(cl), plain_fin)
    with pytest.raises(RuntimeError, match="loc must be"):
        _lib().check(cl.f.lib.slsqp_cl_tube_ratio(cl.f.h, np.empty(B).ctypes.data_as(C.c_void_p), 7))
    cl.run_decoupled(x0, 2, W[:2])
    with pytest.raises(RuntimeError, match="leave no per-batch plan"):
        cl.tube_ratio()
    cl.close()


def test_tube_ratio_of_an_instance_without_a_plan_is_inf():
    """The device of tests/test_gpu_hold_persistent.py: row 0 of instance 1's bounds puts its cart position's upper bound 1e-3 below its state."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B = 6, 4
    x0 = np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.1 * np.arange(B)[:, None])
    g = np.tile(m.g, (B, N + 3, 1))
    g[1, 0, 0] = x0[1, 0] - 1e-3
    cl = _make(m, N, B, bounds=(g, np.tile(m.gf, (B, N + 3, 1))))
    cl.reset(x0)
    r = cl.step(None)
    assert list(r["success"]) == [True, False, True, True]
    t = cl.tube_ratio()
    assert np.isposinf(t[1]) and np.isfinite(t[[0, 2, 3]]).all()
    cl.close()


# ---- 2: off is today ----------------------------------------------------------------------------------------------------------------------------------
def test_theta_inf_is_the_fixed_period_bit_for_bit():
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("rocket")
    N, B, M, steps = 4, 3, 3, 6
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    a = _make(m, N, B)
    plain = a.run_decoupled(x0, steps, W, solve_every=M, persistent_hold=True)
    plain_fin = _final(a)
    a.close()
    b = _make(m, N, B)
    b.f.set_hold_trigger(INF)
    assert b.f.get_hold_trigger() == INF
    off, off_fin = _triggered(m, N, B, M, steps, x0, W, INF, cl=b)
    b.close()
    assert set(off) == set(plain) and "tube_ratio" not in off and "solve_trigger" not in off
    _same(off, plain, skip=("loop_stats",))
    _same(off_fin, plain_fin)
    assert np.array_equal(off["hold_index"], np.tile(np.arange(steps) % M, (B, 1)))


# ---- 3: theta = 0 is M = 1 ----------------------------------------------------------------------------------------------------------------------------
def test_theta_zero_solves_at_every_step():
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("rocket")
    N, B, M, steps = 4, 3, 3, 5
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    a = _make(m, N, B)
    one = a.run_decoupled(x0, steps, W)      # persistent, M = 1
    one_fin = _final(a)
    a.close()
    out, fin = _triggered(m, N, B, M, steps, x0, W, 0.0)
    _same(out, one, skip=("loop_stats",))      # qp_stats included
    _same(fin, one_fin)
    assert "qp_stats" in one and not out["hold_index"].any() and not fin["hold_index"].any()
    assert (out["solve_trigger"][:, 0] == T.SCHEDULED).all() and (out["solve_trigger"][:, 1:] == T.TUBE).all() and (out["tube_ratio"][:, 1:] > 0).all()
    assert out["success"].all()


# ---- 4: the event-triggered run -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,B,M,steps,waves", [
    ("rocket", 4, 3, 4, 8, None),
    ("pendulum", 4, 5, 3, 7, None),
    ("quadrotor", 3, 3, 2, 5, None),
    ("rocket", 4, 70, 3, 6, 7),      # 70 instances on 7 waves: instances queue up and change waves, each on its own schedule
])
def test_event_triggered_run(model, N, B, M, steps, waves):
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    theta = 0.5
    x0, W = _x0_near(m, B), _scaled_W(m, B, steps, M)
    out, fin = _triggered(m, N, B, M, steps, x0, W, theta, waves=waves)
    assert out["loop_stats"]["waves"] == (B if waves is None else waves)
    print("tube_ratio", np.array2string(out["tube_ratio"][:8], precision=4), "solve_trigger", out["solve_trigger"][:8], sep="\n")
    _check_conditions(out, M, theta)
    _check_schedule(out, M, theta)
    _check_qp_stats(out, B, steps)
    which = range(B)
    if B == 70:      # six instances with pairwise different schedules
        seen, which = set(), []
        for b in range(B):
            key = tuple(out["solve_trigger"][b])
            if key not in seen and len(which) < 6:
                seen.add(key)
                which.append(b)
        assert len(which) == 6
    _check_replays(m, N, B, M, steps, x0, W, theta, out, fin, which)


# ---- 5: the variants ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["all", "pp"])
def test_event_triggered_variants(which):
    """k_cl_loop<rocket, 15> (a reference, plant parameters and bounds together) and <rocket, 11> (plant parameters alone)."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("rocket")
    N, B, M, steps, theta = 4, 3, 3, 6, 0.5
    T_rows = steps + N + 1
    kw = {"plant_params": H.spread_params(m, B, 10.0, seed=5)}
    if which == "all":
        refs = [RC.figure8(m, T_rows, z) for z in 0.05 * np.arange(B)]
        kw["reference"] = (np.stack([m.x_ref + 0.2 * (r[0] - m.x_ref) for r in refs]), np.stack([r[1] for r in refs]))
        kw["bounds"] = BC._rows(m, T_rows, {m.nx + j: (None, BC._from(T_rows, 1, 0.9 * m.u_ub[j], np.inf)) for j in range(m.nu)})
    x0, W = _x0_near(m, B), _scaled_W(m, B, steps, M)
    out, fin = _triggered(m, N, B, M, steps, x0, W, theta, **kw)
    print("tube_ratio", np.array2string(out["tube_ratio"], precision=4), "solve_trigger", out["solve_trigger"], sep="\n")
    assert (out["solve_trigger"] == T.HOLD).any() and (out["solve_trigger"][:, 1:] != T.HOLD).any()
    _check_schedule(out, M, theta)
    _check_qp_stats(out, B, steps)
    _check_replays(m, N, B, M, steps, x0, W, theta, out, fin, range(B), **kw)
    assert "model_error" in out


# ---- 6: a failed solve --------------------------------------------------------------------------------------------------------------------------------
def test_failed_solve_is_solved_again_at_the_next_step():
    """Row 0 of instance 1's bounds puts the upper bound of its cart position 1e-3 below its measured state (tests/test_gpu_hold_persistent.py): its
    first solve is refused.  Under the fixed period it would apply the nominal input for M - 1 steps; here its next step is a solve (reason 3).
    The other instances have the bits of a batch without the offset."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, M, steps, theta = 6, 4, 3, 5, 0.5
    x0 = np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.1 * np.arange(B)[:, None])
    W = LO * _seeded_W(m, B, steps)
    g = np.tile(m.g, (B, steps + N + 1, 1))
    gf = np.tile(m.gf, (B, steps + N + 1, 1))
    ref, ref_fin = _triggered(m, N, B, M, steps, x0, W, theta, bounds=(g.copy(), gf))
    g[1, 0, 0] = x0[1, 0] - 1e-3
    out, fin = _triggered(m, N, B, M, steps, x0, W, theta, bounds=(g, gf))
    assert ref["success"][:, 0].all() and not out["success"][1, 0] and out["success"][[0, 2, 3], 0].all()
    assert out["solve_trigger"][1, 1] == T.FAILED and out["hold_index"][1, 1] == 0 and out["tube_ratio"][1, 1] == 0.0
    assert (out["qp_stats"][1, 1, 0, 6] != -1) and out["scp_iterations"][1, 1] >= 0      # it solved
    assert (ref["solve_trigger"][:, 1] != T.FAILED).all()
    if out["success"][1, 1:].all():      # from its first valid plan on it is scheduled like everybody else
        assert (out["solve_trigger"][1, 2:] != T.FAILED).all()
    others = [0, 2, 3]
    for k in out:
        if isinstance(out[k], np.ndarray) and out[k].ndim >= 2 and out[k].shape[0] == B and not k.startswith(("t_", "bounds_")) and k != "constraint_margin":
            assert np.array_equal(out[k][others], ref[k][others], equal_nan=True), k
    for k in fin:
        assert np.array_equal(fin[k][others], ref_fin[k][others]), k
    assert (ref["solve_trigger"] == T.HOLD).any()


# ---- 7: refusals and plumbing -------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_reruns_are_fresh():
    from robust_nonlinear_mpc_amd import get_model
    L = _lib()
    m = get_model("rocket")
    N, B, M, steps, theta = 4, 3, 3, 6, 0.5
    x0, W = _x0_near(m, B), np.ascontiguousarray(_scaled_W(m, B, steps, M))
    fresh, fresh_fin = _triggered(m, N, B, M, steps, x0, W, theta)
    cl = _make(m, N, B)
    cl.reset(x0)

    def state(c):
        return [c.f.get(k, s) for k, s in (("x_meas", (c.m.nx,)), ("nominal_x", (c.N + 1, c.m.nx)), ("nominal_u", (c.N, c.m.nu)))] + [np.array([c.f.get_solve_every(), c.f.get_hold_trigger()])]

    def refused(c, exc, word, call):
        before = state(c)
        with pytest.raises(exc, match=word):
            call()
        assert all(np.array_equal(a, b) for a, b in zip(before, state(c)))

    cl.f.set_hold_trigger(0.25)
    refused(cl, RuntimeError, r"outside \[0, \+inf\]", lambda: cl.f.set_hold_trigger(-0.5))
    refused(cl, RuntimeError, r"outside \[0, \+inf\]", lambda: cl.f.set_hold_trigger(float("nan")))
    assert cl.f.get_hold_trigger() == 0.25
    cl.f.set_solve_every(M)
    wp = W.ctypes.data_as(C.c_void_p)
    cl.f.opts.cl_persistent = 0
    refused(cl, RuntimeError, "persistent launch only", lambda: L.check(cl.f.lib.slsqp_cl_run(cl.f.h, steps, wp, L.HOST, C.byref(cl.f.opts), 8.0, 0.0, None)))
    cl.f.opts.cl_persistent = 1
    refused(cl, RuntimeError, "needs rti = 1 with one fast-SLS step", lambda: L.check(cl.f.lib.slsqp_cl_run_scp(cl.f.h, steps, 3, wp, L.HOST, C.byref(cl.f.opts))))
    cl.f.set_solve_every(1)
    cl.f.set_hold_trigger(None)
    for call in (lambda: cl.run(x0, steps, W, solve_every=M, hold_trigger=theta), lambda: cl.run_on_device(x0, steps, W, solve_every=M, hold_trigger=theta),
                 lambda: cl.run_decoupled(x0, steps, W, solve_every=M, hold_trigger=theta)):
        refused(cl, ValueError, "persistent launch", call)
    refused(cl, ValueError, "hold_trigger must lie in", lambda: cl.run_decoupled(x0, steps, W, solve_every=M, persistent_hold=True, hold_trigger=-1.0))
    # the handle still runs, twice, and gives the bits of a fresh one
    out, fin = _triggered(m, N, B, M, steps, x0, W, theta, cl=cl)
    _same(out, fresh, skip=("loop_stats",))      # (no run before it on this handle: the qp_stats too)
    _same(fin, fresh_fin)
    out, fin = _triggered(m, N, B, M, steps, x0, W, theta, cl=cl)
    _same_rerun(out, fresh)
    _same(fin, fresh_fin)
    with pytest.raises(RuntimeError, match="leave no per-batch plan"):      # as after every persistent run
        cl.f.hold_step(None)
    periodic = cl.run_decoupled(x0, steps, W, solve_every=M, persistent_hold=True)      # the fixed period after the trigger, on the same handle
    assert "tube_ratio" not in periodic and np.array_equal(periodic["hold_index"], np.tile(np.arange(steps) % M, (B, 1)))
    assert (cl.f.get("hold_index", (), np.int32) == (steps - 1) % M).all()
    cl.close()
    # rti = 3 through run_decoupled
    mp = get_model("pendulum")
    cp = _make(mp, 4, 3, rti=None, rti_steps=None)
    cp.reset(_x0(mp, 3))
    refused(cp, RuntimeError, "needs rti = 1 with one fast-SLS step", lambda: cp.run_decoupled(_x0(mp, 3), 4, None, solve_every=2, persistent_hold=True, hold_trigger=theta))
    cp.close()


def test_monte_carlo_with_a_trigger_equals_its_slices():
    from robust_nonlinear_mpc_amd import disturbance_stream, get_model, run_monte_carlo
    m = get_model("rocket")
    N, S, steps, M, theta = 4, 5, 5, 3, 0.5
    x0 = m.x_ref + NEAR["rocket"] * (m.extra["x0"] - m.x_ref)
    with pytest.raises(ValueError, match="persistent launch only"):
        run_monte_carlo(m, N, np.arange(S), steps, x0, slices=2, solve_every=M, hold_trigger=theta)
    mc = run_monte_carlo(m, N, np.arange(S), steps, x0, slices=2, solve_every=M, persistent=True, hold_trigger=theta)
    assert mc["tube_ratio"].shape == (S, steps) and mc["solve_trigger"].shape == (S, steps) and mc["rounds"] == [1, 1]
    assert sum(s["mpc_steps"] for s in mc["loop_stats"]) == S * steps
    for lo, hi in ((0, 2), (2, 5)):      # the slices by hand
        W = np.stack([disturbance_stream(s, steps, m.nx) for s in range(lo, hi)], axis=1)
        part, _ = _triggered(m, N, hi - lo, M, steps, np.tile(x0, (hi - lo, 1)), W, theta)
        for k in part:
            if isinstance(part[k], np.ndarray) and part[k].ndim >= 1 and part[k].shape[0] == hi - lo and not k.startswith("t_"):
                assert np.array_equal(part[k], mc[k][lo:hi], equal_nan=True), k
    _check_schedule(mc, M, theta)

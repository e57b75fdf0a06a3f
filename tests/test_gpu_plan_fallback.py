"""Plan fallback on the device (slsqp_cl_set_plan_fallback, k_cl_plan_fallback, the fallback branch of k_cl_loop's HOLD variants).

A solve is made to fail at a chosen step by a refusal at the strict stage-0 gate (x0_box_tol = 0): one bounded component of the instance's measured
state lies 1e-3 outside its box.  Stepped: x_meas is written through slsqp_set.  Persistent: the displacement goes into the disturbance sample of the
step before through E^-1 (E is checked to be invertible).  The instance gets a constant box of its own close to its trajectory (DELTA above the largest
value the component takes in a run without it), so the kick stays small.  Every test asserts the success pattern it relies on.

Tolerances (tests/test_gpu_hold.py's, the same arithmetic): u0 and hold_xi 1e-11 max(1, |.|inf) against tests/hold_ref.py; x_meas after the plant
step 1e-12 against oracle/dyn_oracle.py's RK4 step; everything else np.array_equal."""
import os

import numpy as np
import pytest

import hold_ref as HR
import plan_fallback_ref as PF
import plant_params_helpers as H

pytestmark = pytest.mark.gpu

TOL_POLICY, TOL_PLANT = 1e-11, 1e-12
DELTA, OUT = 0.05, 1e-3      # the instance's own upper bound above its trajectory; how far outside a kick puts the component
C0 = 0                       # the kicked component: a position of every model, bounded, with a non-zero diagonal entry of E


def _make(m, N, B, **kw):
    from robust_nonlinear_mpc_amd import ClosedLoopMPC
    return ClosedLoopMPC(m, N, B, rti=1, fast_sls_rti_steps=1, **kw)


def _x0(m, B, scale=0.3):
    """Per-instance initial states, as tests/test_gpu_hold.py."""
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


def _same(a, b, skip=()):
    shared = [k for k in a if k in b and not k.startswith("t_") and k not in skip]
    assert shared
    for k in shared:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    return shared


def _own_box(m, B, ub):
    """(g, gf) per instance, one row: the model's box, component C0 of instance b bounded above by ub[b] (a dict)."""
    g, gf = np.tile(m.g, (B, 1, 1)), np.tile(m.gf, (B, 1, 1))
    for b, v in ub.items():
        g[b, 0, C0], gf[b, 0, C0] = v, v
    return g, gf


def _plan(cl):
    m, N, f = cl.m, cl.N, cl.f
    return dict(A=f.get("plan_A", (N, m.nx, m.nx)), Bm=f.get("plan_Bm", (N, m.nx, m.nu)), Kc=f.get("plan_Kc", (N, m.nu, m.nx)),
                backoff_x=f.get("plan_backoff_x", (N + 1, m.nx)), age=f.get("plan_age", (), np.int32))


def _live(cl):
    m, N, f = cl.m, cl.N, cl.f
    return dict(A=f.get("A", (N, m.nx, m.nx)), Bm=f.get("Bm", (N, m.nx, m.nu)), Kc=f.get("Kc", (N, m.nu, m.nx)), backoff_x=f.get("backoff_x", (N + 1, m.nx)),
                nominal_x=f.get("nominal_x", (N + 1, m.nx)), nominal_u=f.get("nominal_u", (N, m.nu)))


def _set_x(cl, x):
    from robust_nonlinear_mpc_amd import _lib as L
    from robust_nonlinear_mpc_amd.fast_sls import _c, _ptr
    x = _c(x)
    L.check(cl.f.lib.slsqp_set(cl.f.h, b"x_meas", _ptr(x), L.HOST))


def _clean_states(m, N, B, steps, x0, W, **kw):
    """x_meas at the start of every step of a stepped run with the option on, and its per-step results; every solve must succeed."""
    cl = _make(m, N, B, plan_fallback=True, **kw)
    cl.reset(x0)
    xs, rs = [], []
    for i in range(steps):
        xs.append(cl.f.get("x_meas", (m.nx,)))
        rs.append(cl.step(W[i]))
        assert rs[-1]["success"].all(), ("the clean run must solve every step", i, rs[-1]["success"])
        assert (rs[-1]["plan_age"] == 0).all() and not rs[-1]["hold_policy"].any()
    cl.close()
    return np.stack(xs), rs


# ---- 1: the stepped loop against numpy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,B", [("pendulum", 4, 3), ("quadrotor", 3, 3), ("rocket", 4, 2)])
def test_stepped_fallback_is_the_restatement(model, N, B):
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    steps, bs = 5, 1      # instance 1 fails at steps 2 and 3 (k = 1, 2: the backup's A_1, B_1, K[1,1]) and recovers at step 4
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    xs, _ = _clean_states(m, N, B, steps, x0, W)
    ub = xs[:, bs, C0].max() + DELTA
    assert ub + OUT < m.x_ub[C0]
    box = _own_box(m, B, {bs: ub})
    xs, clean = _clean_states(m, N, B, steps, x0, W, bounds=box)      # the batch where nobody fails
    others = [b for b in range(B) if b != bs]
    cl = _make(m, N, B, plan_fallback=True, bounds=box)
    assert cl.f.get_plan_fallback()
    cl.reset(x0)
    assert (cl.f.get("plan_age", (), np.int32) == -1).all()
    worst = dict(u0=0.0, xi=0.0, x=0.0)
    saved = None
    for i in range(steps):
        x = cl.f.get("x_meas", (m.nx,))
        if i in (2, 3):
            x[bs, C0] = ub + OUT
            _set_x(cl, x)
        elif i == 4:
            x[bs] = xs[4, bs]      # back inside: where the clean run was
            _set_x(cl, x)
        pre_plan, pre_xi = _plan(cl), cl.f.get("hold_xi", (N + 1, m.nx))
        r = cl.step(W[i])
        live, plan = _live(cl), _plan(cl)
        if i not in (2, 3):
            assert r["success"].all(), (i, r["success"])
            assert (r["plan_age"] == 0).all() and not r["hold_policy"].any()
            for key in ("A", "Bm", "Kc", "backoff_x"):
                assert np.array_equal(plan[key], live[key]), (i, key)      # the snapshot of a solve that succeeded
            if i < 2:
                saved = live
            continue
        k = i - 1
        assert not r["success"][bs] and r["success"][others].all(), (i, r["success"])
        assert r["plan_age"][bs] == k and r["hold_policy"][bs] == 2 and pre_plan["age"][bs] == k - 1
        assert (r["plan_age"][others] == 0).all() and not r["hold_policy"][others].any()
        for key in ("A", "Bm", "Kc", "backoff_x"):
            assert np.array_equal(plan[key][bs], saved[key][bs]) and np.array_equal(pre_plan[key][bs], saved[key][bs]), (i, key)
        assert not np.array_equal(live["A"][bs], plan["A"][bs])      # the failed step did overwrite the live linearisation
        # the live nominal is the backup plan moved k stages: stage 0 is z_k, v_k
        assert np.array_equal(live["nominal_x"][bs, 0], saved["nominal_x"][bs, k]) and np.array_equal(live["nominal_u"][bs, 0], saved["nominal_u"][bs, k])
        K = np.broadcast_to(plan["Kc"][bs][:, None], (N, N + 1, m.nu, m.nx))
        xi0 = pre_xi[bs] if k > 1 else np.zeros((N + 1, m.nx))
        u, _, xi = HR.hold_step(m.model_id, k, x[bs], saved["nominal_x"][bs, k], saved["nominal_u"][bs, k], xi0, plan["A"][bs], plan["Bm"][bs], K, E=m.E, w=W[i][bs])
        _, xn_dev, _ = HR.hold_step(m.model_id, k, x[bs], x[bs], r["u0"][bs], xi0, plan["A"][bs], plan["Bm"][bs], K, E=m.E, w=W[i][bs], hold_policy=0)
        xi_dev = cl.f.get("hold_xi", (N + 1, m.nx))[bs]
        worst["u0"] = max(worst["u0"], np.abs(r["u0"][bs] - u).max() / max(1.0, np.abs(u).max()))
        worst["xi"] = max(worst["xi"], np.abs(xi_dev - xi).max() / max(1.0, np.abs(xi).max()))
        worst["x"] = max(worst["x"], np.abs(r["x_next"][bs] - xn_dev).max())
        print(model, "step", i, "k", k, "worst", worst, "feedback", np.abs(r["u0"][bs] - saved["nominal_u"][bs, k]).max())
        assert worst["u0"] <= TOL_POLICY and worst["xi"] <= TOL_POLICY and worst["x"] < TOL_PLANT, (i, worst)
        assert np.abs(r["u0"][bs] - saved["nominal_u"][bs, k]).max() > 1e-9      # the feedback acts
        assert not xi_dev[0].any() and not xi_dev[k + 1:].any() and xi_dev[k].any()
        # the others are the batch where nobody failed, bit for bit
        assert np.array_equal(r["u0"][others], clean[i]["u0"][others]) and np.array_equal(r["x_next"][others], clean[i]["x_next"][others])
        assert np.array_equal(r["nominal_x"][others], clean[i]["nominal_x"][others])
    cl.close()


# ---- 2: the age cap -----------------------------------------------------------------------------------------------------------------------------------
def test_age_cap_and_no_backup():
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, steps, bs = 3, 3, 5, 1
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    xs, _ = _clean_states(m, N, B, steps, x0, W)
    ub = np.abs(xs[:, bs, C0]).max() + DELTA
    box = _own_box(m, B, {bs: ub})
    cl = _make(m, N, B, plan_fallback=True, bounds=box)
    cl.reset(x0)
    want = {2: (2, 1), 3: (2, 2), 4: (0, -1)}      # step: (policy code, age): k = 1 and 2 run the policy, the third failure finds no row left
    for i in range(steps):
        x = cl.f.get("x_meas", (m.nx,))
        if i in want:
            x[bs, C0] = ub + OUT
            _set_x(cl, x)
        nom_u, xi_pre = cl.f.get("nominal_u", (N, m.nu)), cl.f.get("hold_xi", (N + 1, m.nx))
        r = cl.step(W[i])
        if i not in want:
            assert r["success"].all() and (r["plan_age"] == 0).all()
            continue
        assert not r["success"][bs] and (r["hold_policy"][bs], r["plan_age"][bs]) == want[i], (i, r["hold_policy"], r["plan_age"])
        if want[i][0] == 0:      # today's behaviour: the nominal input of the shifted plan, xi stays
            assert np.array_equal(r["u0"][bs], nom_u[bs, 1]) and np.array_equal(cl.f.get("hold_xi", (N + 1, m.nx))[bs], xi_pre[bs])
        else:
            assert not np.array_equal(r["u0"][bs], nom_u[bs, 1])
    cl.close()
    # a failure at step 0: no backup yet
    cl = _make(m, N, B, plan_fallback=True, bounds=box)
    cl.reset(x0)
    x = cl.f.get("x_meas", (m.nx,))
    x[bs, C0] = ub + OUT
    _set_x(cl, x)
    nom_u = cl.f.get("nominal_u", (N, m.nu))
    r = cl.step(W[0])
    assert not r["success"][bs] and r["success"][[0, 2]].all()
    assert r["hold_policy"][bs] == 0 and r["plan_age"][bs] == -1 and np.array_equal(r["u0"][bs], nom_u[bs, 0])
    assert (r["plan_age"][[0, 2]] == 0).all()
    cl.close()


# ---- 3: the persistent launch is the stepped loop ---------------------------------------------------------------------------------------------------
def _run(m, N, B, M, steps, x0, W, persistent, waves=None, theta=None, **kw):
    """One run with the option on: result, final state.  persistent: run_decoupled (persistent_hold for M > 1), else run_on_device."""
    cl = _make(m, N, B, plan_fallback=True, **kw)
    if waves is not None:
        os.environ["SLSQP_LOOP_WAVES"] = str(waves)
    try:
        if persistent:
            out = cl.run_decoupled(x0, steps, W, solve_every=M, persistent_hold=M > 1, **({} if theta is None else dict(hold_trigger=theta)))
        else:
            out = cl.run_on_device(x0, steps, W, solve_every=M)
    finally:
        os.environ.pop("SLSQP_LOOP_WAVES", None)
    f = cl.f
    fin = dict(x_meas=f.get("x_meas", (m.nx,)), nominal_x=f.get("nominal_x", (N + 1, m.nx)), u0=f.get("u0", (m.nu,)), hold_xi=f.get("hold_xi", (N + 1, m.nx)),
               plan_age=f.get("plan_age", (), np.int32), plan_A=f.get("plan_A", (N, m.nx, m.nx)), plan_Kc=f.get("plan_Kc", (N, m.nu, m.nx)),
               plan_backoff_x=f.get("plan_backoff_x", (N + 1, m.nx)))
    cl.close()
    return out, fin


def _kicked_W(m, N, B, M, steps, x0, W, fails, back, run=None, **kw):
    """W with the kicks that make instance b fail at the steps fails[b] (component C0 OUT above the instance's own bound) and put it back where the
    clean run was at step back[b]; the box that goes with it.  Built step by step: x_meas at step t is the final state of a run of t steps."""
    run = run or (lambda t, Wk, **k2: _run(m, N, B, M, t, x0, Wk[:t], False, **k2)[1]["x_meas"])
    E = np.asarray(m.E, dtype=float)
    assert np.linalg.matrix_rank(E) == m.nx
    T = max(max(back.values()), max(max(v) for v in fails.values()))
    clean = np.stack([x0] + [run(t, W, **kw) for t in range(1, T + 1)])      # (T + 1, B, nx)
    ub = {b: clean[:, b, C0].max() + DELTA for b in fails}
    box = _own_box(m, B, ub)
    clean = np.stack([x0] + [run(t, W, bounds=box, **kw) for t in range(1, T + 1)])
    Wk = W.copy()
    for t in range(1, T + 1):
        todo = [b for b in fails if t in fails[b] or t == back[b]]
        if not todo:
            continue
        x = run(t, Wk, bounds=box, **kw)
        for b in todo:
            d = np.zeros(m.nx)
            d[C0] = (ub[b] + OUT if t in fails[b] else clean[t, b, C0]) - x[b, C0]
            Wk[t - 1, b] += np.linalg.solve(E, d)
    return Wk, box


def _check_pattern(out, fails, back, N, M, steps, B):
    """The success pattern the comparison relies on: exactly the kicked solves failed, and ages and policy codes are those of the numpy restatement
    (tests/plan_fallback_ref.py) -- the kicked solves ran the backup's policy (code 2) at the age the schedule gives."""
    ok, pol, age = out["success"], out["hold_policy"], out["plan_age"]
    solve = out["hold_index"] == 0
    failed = np.zeros((B, steps), dtype=bool)
    for b, at in fails.items():
        failed[b, list(at)] = True
    assert np.array_equal(solve, np.tile(np.arange(steps) % M == 0, (B, 1)))
    assert np.array_equal(ok[solve], ~failed[solve]), ("success", ok)
    _, code, want_age = PF.run(N, out["hold_index"], ok)
    assert np.array_equal(age, want_age), ("plan_age", age, want_age)
    assert np.array_equal(pol, code), ("hold_policy", pol, code)
    assert (pol[failed] == 2).all() and int((pol == 2).sum()) == sum(len(v) for v in fails.values())


@pytest.mark.parametrize("model,N,B,M,steps,fails,back,waves,pp", [
    ("pendulum", 4, 3, 1, 6, {1: (2, 3)}, {1: 4}, None, False),
    ("pendulum", 6, 3, 3, 8, {1: (3,)}, {1: 6}, None, False),      # the hold steps 4 and 5 continue the backup's policy at k = 4, 5
    ("quadrotor", 3, 3, 2, 5, {2: (2,)}, {2: 4}, None, False),
    ("rocket", 4, 2, 1, 5, {0: (2, 3)}, {0: 4}, None, False),
    ("rocket", 4, 70, 1, 5, {3: (2,), 17: (2, 3), 40: (1, 2), 69: (3,)}, {3: 3, 17: 4, 40: 3, 69: 4}, 7, False),      # 7 waves: an instance fails on one wave and goes on on another
    ("pendulum", 4, 3, 1, 5, {1: (2, 3)}, {1: 4}, None, True),      # plant parameters and bounds: VAR 15
])
def test_persistent_fallback_is_the_stepped_loop(model, N, B, M, steps, fails, back, waves, pp):
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    kw = dict(plant_params=H.spread_params(m, B, 3.0, 5)) if pp else {}
    Wk, box = _kicked_W(m, N, B, M, steps, x0, W, fails, back, **kw)
    ref, ref_fin = _run(m, N, B, M, steps, x0, Wk, False, bounds=box, **kw)
    _check_pattern(ref, fails, back, N, M, steps, B)
    out, fin = _run(m, N, B, M, steps, x0, Wk, True, waves=waves, bounds=box, **kw)
    shared = _same(out, ref)
    assert {"plan_age", "hold_policy", "hold_index", "success", "state_trajectory", "input_trajectory"} <= set(shared)
    _same(fin, ref_fin)
    assert out["loop_stats"]["waves"] == (B if waves is None else waves) and out["loop_stats"]["mpc_steps"] == B * steps


def test_triggered_run_solves_again_after_a_fallback():
    """A finite theta: the step after a failed solve is a solve again (code 3), and the failed solve itself ran the backup's policy (code 2)."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, M, steps, bs, theta = 6, 3, 3, 7, 1, 1e9
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    run = lambda t, Wk, **k2: _run(m, N, B, M, t, x0, Wk[:t], True, theta=theta, **k2)[1]["x_meas"]      # noqa: E731
    Wk, box = _kicked_W(m, N, B, M, steps, x0, W, {bs: (3,)}, {bs: 4}, run=run)
    out, _ = _run(m, N, B, M, steps, x0, Wk, True, theta=theta, bounds=box)
    print("hold_index", out["hold_index"][bs], "trigger", out["solve_trigger"][bs], "policy", out["hold_policy"][bs], "age", out["plan_age"][bs], "success", out["success"][bs])
    assert out["hold_index"][bs, 3] == 0 and not out["success"][bs, 3] and out["hold_policy"][bs, 3] == 2 and out["plan_age"][bs, 3] == 3
    assert out["solve_trigger"][bs, 4] == 3 and out["hold_index"][bs, 4] == 0 and out["success"][bs, 4] and out["plan_age"][bs, 4] == 0


# ---- 4: off is today ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persistent,M", [(False, 1), (False, 3), (True, 1), (True, 3)])
def test_off_is_today_and_the_snapshot_perturbs_nothing(persistent, M):
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, steps = 4, 3, 5
    x0, W = _x0(m, B), _seeded_W(m, B, steps)

    def run(ctor, setter=None):
        cl = _make(m, N, B, **ctor)
        if setter is not None:
            cl.f.set_plan_fallback(setter)
        out = cl.run_decoupled(x0, steps, W, solve_every=M, persistent_hold=M > 1) if persistent else cl.run_on_device(x0, steps, W, solve_every=M)
        out["final_x"], out["final_xi"] = cl.f.get("x_meas", (m.nx,)), cl.f.get("hold_xi", (N + 1, m.nx))
        cl.close()
        return out
    never, zero, on = run({}), run({}, 0), run(dict(plan_fallback=True))
    assert set(never) == set(zero) and "plan_age" not in never
    skip = ("loop_stats", "rounds")      # (wave statistics of a launch: clock readings)
    _same(zero, never, skip)
    assert on["success"].all()      # no solve fails: the option only takes its snapshots
    shared = _same(on, never, skip)
    assert {"state_trajectory", "input_trajectory", "final_x", "final_xi", "success"} <= set(shared) and (M == 1 or "hold_policy" in shared)
    assert np.array_equal(on["plan_age"], np.tile(np.arange(steps) % M, (B, 1))) and np.array_equal(on["hold_index"], on["plan_age"])


# ---- 5: refusals and plumbing ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model
    m = get_model("pendulum")
    N, B, steps = 4, 3, 3
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    cl = _make(m, N, B)
    for bad in (2, -1, 7):
        with pytest.raises(RuntimeError, match="neither 0"):
            cl.f.set_plan_fallback(bad)
        assert cl.f.get_plan_fallback() is False
    with pytest.raises(ValueError):
        cl.f.set_plan_fallback("yes")
    cl.f.set_plan_fallback(True)
    assert cl.f.get_plan_fallback() is True
    cl.f.set_plan_fallback(0)
    assert cl.f.get_plan_fallback() is False and (cl.f.get("plan_age", (), np.int32) == -1).all() and not cl.f.get("plan_A", (N, m.nx, m.nx)).any()
    cl.close()
    # rti = 3 / two fast-SLS steps: refused at the call that would need the option, nothing stepped
    for rti, rs in ((3, 1), (1, 2)):
        cl = ClosedLoopMPC(m, N, B, rti=rti, fast_sls_rti_steps=rs, plan_fallback=True)
        cl.reset(x0)
        with pytest.raises(RuntimeError, match="needs rti = 1 with one fast-SLS step"):
            cl.step(W[0])
        assert np.array_equal(cl.f.get("x_meas", (m.nx,)), x0)
        with pytest.raises(RuntimeError, match="needs rti = 1 with one fast-SLS step"):
            cl.run_decoupled(x0, steps, W)
        cl.close()
    # the round-based loop
    cl = _make(m, N, B, plan_fallback=True)
    cl.f.opts.cl_persistent = 0
    with pytest.raises(RuntimeError, match="persistent launch only"):
        cl.run_decoupled(x0, steps, W)
    cl.close()


def test_rerun_on_a_used_handle():
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, M, steps, fails, back = 4, 3, 1, 5, {1: (2, 3)}, {1: 4}
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    Wk, box = _kicked_W(m, N, B, M, steps, x0, W, fails, back)
    fresh, _ = _run(m, N, B, M, steps, x0, Wk, True, bounds=box)
    _check_pattern(fresh, fails, back, N, M, steps, B)
    cl = _make(m, N, B, plan_fallback=True, bounds=box)
    cl.run_decoupled(x0, steps, W)
    assert (cl.f.get("plan_age", (), np.int32) == 0).all()
    again = cl.run_decoupled(x0, steps, Wk)      # slsqp_cl_init has set every age back to -1: the pattern is the fresh handle's
    cl.close()
    _same(again, fresh, skip=("loop_stats", "qp_stats"))      # (step 0's qp_stats: the existing rule, tests/test_gpu_hold_persistent.py)
    assert np.array_equal(again["qp_stats"][:, 1:], fresh["qp_stats"][:, 1:]) and np.array_equal(again["qp_stats"][:, 0, :, 6], fresh["qp_stats"][:, 0, :, 6])


def test_monte_carlo_equals_its_slices():
    from robust_nonlinear_mpc_amd import get_model, run_monte_carlo
    m = get_model("rocket")
    N, S, steps = 4, 6, 4
    x0 = m.x_ref + 0.3 * (m.extra["x0"] - m.x_ref)
    one = run_monte_carlo(m, N, np.arange(S), steps, x0, plan_fallback=True)
    two = run_monte_carlo(m, N, np.arange(S), steps, x0, plan_fallback=True, slices=2)
    off = run_monte_carlo(m, N, np.arange(S), steps, x0)
    assert "plan_age" in one and one["plan_age"].shape == (S, steps) and "plan_age" not in off
    _same(two, one, skip=("rounds", "loop_stats", "seeds"))
    for a in (np.arange(0, 3), np.arange(3, 6)):
        part = run_monte_carlo(m, N, a, steps, x0, plan_fallback=True)
        for k in ("state_trajectory", "input_trajectory", "plan_age", "hold_policy", "success"):
            assert np.array_equal(part[k], one[k][a], equal_nan=True), k

"""Measurement noise in the on-device closed loops (slsqp_cl_set_meas_noise) on the GPU, at the suite's smallest shapes
(pendulum N = 3, B = 5, 3 steps; rocket N = 4, B = 6, 4 steps; the persistent launches with 2 waves).  The tables are per instance with T = 2 rows
(the held row is in use from step 2 on), entries inside E[0]'s box.  Comparisons are np.array_equal unless said otherwise.

  1. the rule: measured_trajectory = state_trajectory + row min(s, T - 1), x_meas / x_plant after the run likewise; once more shared with T = 1;
  2. the plant runs on the truth: state_trajectory[s + 1] against the host's ddyn(_p) at (state_trajectory[s], input_trajectory[s]) plus E w_s, 1e-12
     (the tolerance of tests/test_gpu_plant_params.py for this comparison), with and without plant parameters;
  3. the controller runs on the measurement: a fresh handle with the option off, given the recorded measurement before every slsqp_cl_step, gives every
     controller output of every step bit for bit;
  4. routes: with the option on every route equals the stepped loop in every shared key and the final state, alone, with the adversary (whose w_applied
     is adversary_ref on the TRUE state) and with plant parameters, bounds and a reference; the event-triggered run against the stepped replay of each
     instance's own schedule;
  5. off is off: never set = set and cleared = run under the option, then cleared; an all-zero table gives the plain run's values;
  6. a non-zero table changes the inputs;
  7. refusals, log_plant_state without a log, x_plant before slsqp_cl_init, a setter call inside a run, a second run on a used handle.

Where the plain run and the all-zero table are compared, `state_trajectory` is the one shared key whose meaning the option changes: the plain run's
is log_state (stage 0 of the nominal after the step, x_nom0 - fl(x_nom0 - x) after a solve that succeeded), the option's is the true state.  So the
zero-table run's log_state is compared with the plain run's `state_trajectory` bit for bit, and its true trajectory against that within the rounding
of those two operations (test_off_is_off states the bound)."""
import ctypes as C

import numpy as np
import pytest

import adversary_ref as AR
import loop_args_runs as R
import meas_noise_ref as MR
import plant_params_helpers as H
import test_gpu_adversary as TA
import test_gpu_hold_trigger as HT

pytestmark = pytest.mark.gpu

_setup = TA._setup
CTRL_KEYS = ("input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x", "backoff_trajectory_u", "success", "scp_iterations",
             "primal_infeasibility", "x0_violation", "qp_stats")


def _same(a, b, fa=None, fb=None, what="", skip=()):
    """Every shared key but the timings, and the final state where given; the assertion message carries what differs and by how much."""
    keys = [k for k in a if k in b and k not in TA.TIMING_KEYS and k not in skip]
    assert "success" in keys and "input_trajectory" in keys
    bad = {k: d for k in keys for d in [TA._differing(a[k], b[k])] if d is not None}
    if fa is not None:
        bad.update({"final " + k: d for k in fa if k in fb for d in [TA._differing(fa[k], fb[k])] if d is not None})
    print(what, "compared", len(keys), "keys; differing:", bad)
    assert not bad, (what, bad)
    return keys


def _table(m, B, T=2, per=True, amp=1.0):
    """amp E[0] v, v the seeds' own unit streams: inside the set the stage-0 column assumes (a few 1e-3 for the pendulum's E = 0.003 I)."""
    from robust_nonlinear_mpc_amd import meas_noise_table, measurement_stream
    v = np.stack([measurement_stream(100 + b, T, m.nw) for b in range(B)])
    t = meas_noise_table(m, v if per else v[0], amp)
    assert np.all(np.abs(np.linalg.solve(np.asarray(m.E, dtype=float), t.reshape(-1, m.nx).T)) <= amp * (1.0 + 1e-12)) and t.any()
    return t


def _make(m, N, B, table=None, adversary=None, tune=None, **kw):
    from robust_nonlinear_mpc_amd import ClosedLoopMPC
    cl = ClosedLoopMPC(m, N, B, **kw)
    for k, v in (tune or {}).items():
        setattr(cl.f.opts, k, v)
    if table is not None:
        cl.set_meas_noise(table)
    if adversary is not None:
        cl.set_adversary(adversary)
    return cl


def _final(cl):
    fin = R.final(cl)
    fin["x_plant"] = cl.f.get("x_plant", (cl.m.nx,))
    return fin


def _stepwise(cl, steps, x0, W, **kw):
    out, _ = R.stepwise(cl, steps, x0, W, close=False, **kw)
    return out, _final(cl)


def _decoupled(cl, steps, x0, W, **kw):
    out, _ = R.decoupled(cl, steps, x0, W, close=False, **kw)
    return out, _final(cl)


def _on_device(cl, steps, x0, W, **kw):
    return cl.run_on_device(x0, steps, W, **kw), _final(cl)


def _host_run(cl, steps, x0, W, **kw):
    kw.pop("continuation", None)
    return cl.run(x0, steps, W, **kw), _final(cl)


PEND = dict(rti=3, fast_sls_rti_steps=2)
CONV = dict(rti=2, fast_sls_rti_steps=None)
# route: (plant, constructor keywords, runner, run keywords, the stepped route it must equal)
ROUTES = {
    "step_pendulum": ("pendulum", PEND, _stepwise, {}, None),
    "step_rocket": ("rocket", {}, _stepwise, {}, None),
    "step_converge": ("pendulum", CONV, _stepwise, {}, None),
    "solve_every_stepped": ("rocket", {}, _on_device, dict(solve_every=2), None),
    "plan_fallback_stepped": ("rocket", dict(plan_fallback=True), _on_device, {}, None),
    "plan_fallback_hold_stepped": ("rocket", dict(plan_fallback=True), _on_device, dict(solve_every=2), None),
    "run": ("pendulum", PEND, _host_run, {}, "step_pendulum"),
    "run_on_device": ("rocket", {}, _on_device, {}, "step_rocket"),
    "rounds": ("rocket", dict(tune=dict(cl_persistent=0)), _decoupled, {}, "step_rocket"),
    "k_cl_loop": ("rocket", {}, _decoupled, {}, "step_rocket"),
    "k_cl_loop_scp": ("pendulum", PEND, _decoupled, {}, "step_pendulum"),
    "sls_converge": ("pendulum", CONV, _decoupled, dict(persistent_converge=True), "step_converge"),
    "solve_every_persistent": ("rocket", {}, _decoupled, dict(solve_every=2, persistent_hold=True), "solve_every_stepped"),
    "plan_fallback": ("rocket", dict(plan_fallback=True), _decoupled, {}, "plan_fallback_stepped"),
    "plan_fallback_hold": ("rocket", dict(plan_fallback=True), _decoupled, dict(solve_every=2, persistent_hold=True), "plan_fallback_hold_stepped"),
    "hold_trigger": ("rocket", {}, _decoupled, dict(solve_every=3, persistent_hold=True, hold_trigger=0.5), None),
}
PAIRED = [r for r, v in ROUTES.items() if v[4]]
_cache = {}


def _route(route, table="per", adversary=None, then=None, cached=False, **opt):
    """One run of a route; table: "per" (per instance, T = 2), "zero", None (option never set) or an array.  (out, fin, W, table)."""
    cached = cached and isinstance(table, (str, type(None)))
    key = (route, table if cached else None, adversary)
    if cached and not opt and key in _cache:
        return _cache[key]
    name, ckw, runner, rkw, _ = ROUTES[route]
    m, N, B, steps, x0, W, kw = _setup(name)
    tab = _table(m, B) if isinstance(table, str) and table == "per" else np.zeros((B, 2, m.nx)) if isinstance(table, str) else table
    cl = _make(m, N, B, tab, adversary, **ckw, **opt)
    try:
        out, fin = runner(cl, steps, x0, W, **kw, **rkw)
        if then:
            then(cl)
    finally:
        cl.close()
    res = (out, fin, W, tab)
    if cached and not opt:
        _cache[key] = res
    return res


def _true_start(name, x0):
    """Where the plant of a run of `name` starts: x0, or what the last stage of reset()'s continuation makes of it (its own expression, at s = 1)."""
    m, kw = _setup(name)[0], _setup(name)[6]
    K = kw.get("continuation", 1)
    return x0 if K == 1 else m.x_ref + (x0 - m.x_ref) * (K / K)


def _check_rule(out, fin, tab, x0):
    X, Y = out["state_trajectory"], out["measured_trajectory"]
    steps = X.shape[2]
    assert np.array_equal(X[:, :, 0], x0)      # slsqp_cl_init took the true state
    assert np.array_equal(Y, MR.measured_trajectory(X, tab))
    assert np.array_equal(fin["x_meas"], MR.measure(fin["x_plant"], tab, steps))
    assert np.array_equal(out["meas_noise"], tab)


# ---- 1: the rule ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["step_pendulum", "k_cl_loop", "run"])
def test_measurement_is_the_true_state_plus_the_row(route):
    out, fin, W, tab = _route(route, cached=True)
    x0 = _true_start(ROUTES[route][0], _setup(ROUTES[route][0])[4])
    _check_rule(out, fin, tab, x0)
    assert (out["measured_trajectory"] != out["state_trajectory"]).any(axis=1).all()      # every instance, every step


@pytest.mark.parametrize("route", ["step_rocket", "k_cl_loop_scp"])
def test_shared_constant_bias(route):
    m, N, B, steps, x0, W, kw = _setup(ROUTES[route][0])
    tab = _table(m, B, T=1, per=False)
    assert tab.shape == (1, m.nx)

    def served(cl):
        assert np.array_equal(cl.f.get("meas_noise", (1, m.nx)), np.tile(tab, (B, 1, 1)))      # a shared table repeated
    out, fin, _, _ = _route(route, table=tab, then=served)
    _check_rule(out, fin, tab, _true_start(ROUTES[route][0], x0))


# ---- 2: the plant runs on the truth --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,pp", [("step_rocket", 0), ("k_cl_loop", 0), ("k_cl_loop", 1), ("step_pendulum", 1)])
def test_plant_steps_from_the_true_state(route, pp):
    m, N, B, steps, x0, W, kw = _setup(ROUTES[route][0])
    mk = R.option_state(m, B, (0, pp, 0))
    out, fin, _, tab = _route(route, **mk) if pp else _route(route, cached=True)
    X, U = out["state_trajectory"], out["input_trajectory"]
    worst, moved = 0.0, 0.0
    for s in range(steps - 1):
        for b in range(B):
            f = H.host_ddyn_p(m.model_id, X[b, :, s], U[b, :, s], mk["plant_params"][b]) if pp else H.host_ddyn_c(m.model_id, X[b, :, s], U[b, :, s])
            worst = max(worst, np.abs(X[b, :, s + 1] - (f + m.E @ W[s][b])).max())
            g = H.host_ddyn_c(m.model_id, out["measured_trajectory"][b, :, s], U[b, :, s])      # (what a plant that stepped from the measurement would give)
            moved = max(moved, np.abs(g - f).max())
    print(route, pp, "largest |x+ - (ddyn(x, u) + E w)|", worst, "; a step from the measurement would differ by", moved)
    assert worst < 1e-12 and moved > 1e-6
    if pp:
        assert out["model_error"].any()


# ---- 3: the controller runs on the measurement (replay) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pendulum", "rocket"])
def test_replay_of_the_measurements_with_the_option_off(name):
    m, N, B, steps, x0, W, _ = _setup(name)
    kw = dict(solve_nominal=True)      # (no continuation: its stages are taken between the neutral point and the state it is GIVEN)
    ckw = PEND if name == "pendulum" else {}
    cl = _make(m, N, B, _table(m, B), **ckw)
    try:
        noisy, _ = _stepwise(cl, steps, x0, W, **kw)
    finally:
        cl.close()
    Y = noisy["measured_trajectory"]
    L = __import__("robust_nonlinear_mpc_amd")._lib
    cl = _make(m, N, B, None, **ckw)
    try:
        L.check(cl.f.lib.slsqp_cl_log(cl.f.h, steps))
        cl.reset(Y[:, :, 0], **kw)
        stats = []
        for i in range(steps):
            y = np.ascontiguousarray(Y[:, :, i])
            L.check(cl.f.lib.slsqp_set(cl.f.h, b"x_meas", y.ctypes.data_as(C.c_void_p), L.HOST))
            cl.step(W[i], fetch=False)
            stats.append(cl.f.get("qp_stats", (2, 8), np.int32))
        z = np.zeros((steps, 1))
        rep = cl._log_result(steps, z, z, z)
        rep["qp_stats"] = np.stack(stats, axis=1)
    finally:
        cl.close()
    assert "measured_trajectory" not in rep
    bad = {k: TA._differing(noisy[k], rep[k]) for k in CTRL_KEYS if TA._differing(noisy[k], rep[k]) is not None}
    assert not bad, bad
    assert R.real_work(noisy)


# ---- 4: routes -----------------------------------------------------------------------------------------------------------------------------------------
def _w_expected(m, out, W, bounds=None, Xref=None):
    X = out["state_trajectory"]      # the TRUE states
    return np.stack([AR.applied_batch(AR.NEAREST_BOUND, 1.0, None, X[:, :, t], m.E, W[t], s=t, g=m.g, bounds=bounds, Xref=Xref) for t in range(X.shape[2])])


@pytest.mark.parametrize("adversary", [None, "nearest_bound"], ids=["alone", "adversary"])
@pytest.mark.parametrize("route", PAIRED)
def test_route_equals_the_stepped_loop(route, adversary):
    a, fa, W, tab = _route(route, adversary=adversary, cached=True)
    b, fb, _, _ = _route(ROUTES[route][4], adversary=adversary, cached=True)
    keys = _same(a, b, fa, fb, (route, adversary))
    assert "measured_trajectory" in keys and "meas_noise" in keys
    m, _, _, _, x0, _, _ = _setup(ROUTES[route][0])
    _check_rule(a, fa, tab, _true_start(ROUTES[route][0], x0))
    if adversary:
        assert "w_applied" in keys and np.array_equal(a["w_applied"], _w_expected(m, a, W))      # nature reads the true state


@pytest.mark.parametrize("name", ["pendulum", "rocket"])
@pytest.mark.parametrize("state", [(0, 1, 0), (0, 0, 1), (1, 0, 0), (1, 1, 1)], ids=["params", "bounds", "reference", "all"])
def test_persistent_launch_equals_the_stepped_loop_with_the_other_options(name, state):
    m, N, B, steps, x0, W, kw = _setup(name)
    mk = R.option_state(m, B, state)
    adversary = "nearest_bound" if state == (1, 1, 1) else None
    a, fa, _, tab = _route("step_" + name, adversary=adversary, **mk)
    b, fb, _, _ = _route("k_cl_loop" if name == "rocket" else "k_cl_loop_scp", adversary=adversary, **mk)
    keys = _same(a, b, fa, fb, (name, state))
    assert ("model_error" in keys) == bool(state[1]) and ("constraint_margin" in keys) == bool(state[2]) and "measured_trajectory" in keys
    _check_rule(b, fb, tab, _true_start(name, x0))
    if adversary:
        assert np.array_equal(a["w_applied"], _w_expected(m, a, W, bounds=mk["bounds"][0], Xref=mk["reference"][0]))


def test_event_triggered_run_against_the_replay_of_each_schedule():
    """The trigger reads the measurement: every instance's triggered run equals the stepped replay of its own schedule, decided from x_meas."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("rocket")
    N, B, M, steps, theta = 4, 3, 3, 6, 0.5
    x0, W = HT._x0_near(m, B), HT._scaled_W(m, B, steps, M)
    tab = _table(m, B, amp=0.25)
    out, fin = HT._triggered(m, N, B, M, steps, x0, W, theta, waves=2, meas_noise=tab)
    assert np.array_equal(out["measured_trajectory"], MR.measured_trajectory(out["state_trajectory"], tab))
    assert (out["hold_index"] > 0).any() and (out["solve_trigger"][:, 1:] != 0).any()
    HT._check_replays(m, N, B, M, steps, x0, W, theta, out, fin, range(B), meas_noise=tab)


# ---- 5: off is off -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_off_is_off(route):
    plain, fplain, W, _ = _route(route, table=None, cached=True)
    assert "measured_trajectory" not in plain and np.array_equal(fplain["x_plant"], fplain["x_meas"])
    name, ckw, runner, rkw, _ = ROUTES[route]
    m, N, B, steps, x0, _, kw = _setup(name)
    cl = _make(m, N, B, _table(m, B), **ckw)      # set and cleared: a handle that never had it
    try:
        cl.set_meas_noise(None)
        out, fin = runner(cl, steps, x0, W, **kw, **rkw)
    finally:
        cl.close()
    assert "measured_trajectory" not in out
    _same(out, plain, fin, fplain, (route, "cleared"))
    cl = _make(m, N, B, _table(m, B), **ckw)      # a run under the option, then cleared on the same handle
    try:
        noisy, _ = runner(cl, steps, x0, W, **kw, **rkw)
        cl.set_meas_noise(None)
        out, fin = runner(cl, steps, x0, W, **kw, **rkw)
        if route != "run":
            assert np.array_equal(cl.f.get("log_plant_state", (steps, m.nx)), cl.f.get("log_state", (steps, m.nx)))      # off: a copy of log_state
    finally:
        cl.close()
    _same(out, plain, fin, fplain, (route, "run, then cleared"), skip=("qp_stats",))      # (step 0's qp_stats of a used handle: tests/test_gpu_hold_persistent.py)
    assert np.array_equal(fin["x_plant"], fplain["x_plant"])
    # 6: it did something
    assert (noisy["input_trajectory"] != plain["input_trajectory"]).any() and (noisy["measured_trajectory"] != noisy["state_trajectory"]).any()
    pinned_log = {}

    def keep_log_state(cl):
        if route != "run":      # (run() keeps no device-side log)
            pinned_log["log_state"] = cl.f.get("log_state", (steps, m.nx)).transpose(0, 2, 1)
    zero, fzero, _, _ = _route(route, table="zero", then=keep_log_state)      # an all-zero table
    ok = plain["success"]
    assert np.array_equal(zero["measured_trajectory"], zero["state_trajectory"])
    keys = _same(zero, plain, None, None, (route, "zero table"), skip=("state_trajectory",))
    for k in R.FIN_KEYS:
        assert np.array_equal(fzero[k], fplain[k], equal_nan=True), (route, k)
    assert np.array_equal(fzero["x_plant"], fplain["x_meas"])
    # `state_trajectory` is the one shared key whose MEANING the option changes: the plain run's is log_state, stage 0 of the nominal after the step.
    # log_state itself keeps its bits ...
    if pinned_log:
        assert np.array_equal(pinned_log["log_state"], plain["state_trajectory"])
    # ... and the truth is that value up to the rounding of the pin: a solve that succeeds leaves x_nom0 - fl(x_nom0 - x) there, two correctly rounded
    # fp64 operations, |error| <= 2^-53 (|x_nom0 - x| + |x|) (1 + 2^-53) -- exact wherever the subtraction is (Sterbenz), as on the pendulum; further
    # SCP iterations of the step start closer to x and stay inside the bound.  x_nom0 of step s >= 1 is stage 1 of step s - 1's nominal.  A hold
    # step logs x_meas itself; a solve that failed logs the prediction and is left out.
    held = plain["hold_index"] > 0 if "hold_index" in plain else np.zeros_like(ok)
    X, P = zero["state_trajectory"], plain["state_trajectory"]
    ratio = 0.0
    for s in range(1, steps):
        pred = plain["nominal_trajectory_x"][:, :, 1, s - 1]
        bound = 2.0 ** -52 * (np.abs(pred - X[:, :, s]) + np.abs(X[:, :, s]))
        err = np.abs(X[:, :, s] - P[:, :, s])
        sel = ok[:, s] & ~held[:, s]
        assert np.all(err[sel] <= bound[sel]), (route, s, err[sel].max())
        assert np.array_equal(X[held[:, s], :, s], P[held[:, s], :, s])
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = max(ratio, float(np.nanmax(np.where(sel[:, None] & (bound > 0), err / bound, 0.0), initial=0.0)))
    print(route, "truth against log_state: largest error / bound", ratio, "; entries that differ", int((X != P).sum()))
    assert np.array_equal(X[:, :, 0], _true_start(name, x0)) and (ok | held)[:, 1:].any()
    assert "success" in keys


# ---- 7: refusals and plumbing --------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_plumbing():
    import types
    from robust_nonlinear_mpc_amd import BatchedFastSLS
    m, N, B, steps, x0, W, kw = _setup("pendulum")
    cl = _make(m, N, B, None, **PEND)
    lib, h = cl.f.lib, cl.f.h
    dp = C.POINTER(C.c_double)
    try:
        # before any slsqp_cl_init: the one state
        assert np.array_equal(cl.f.get("x_plant", (m.nx,)), cl.f.get("x_meas", (m.nx,)))
        with pytest.raises(RuntimeError, match="unknown result name: log_plant_state"):
            cl.f.get("log_plant_state", (steps, m.nx))
        tab = _table(m, B)
        cl.set_meas_noise(tab)
        good = np.ascontiguousarray(tab)
        ptr = good.ctypes.data_as(dp)

        def refused(Nm, T, per, loc, words):
            assert lib.slsqp_cl_set_meas_noise(h, Nm, T, per, loc) != 0
            msg = lib.slsqp_last_error().decode()
            assert "slsqp_cl_set_meas_noise" in msg and words in msg, msg
        refused(ptr, -1, 1, 0, "T = -1")
        refused(ptr, 0, 1, 0, "T = 0")
        refused(None, 2, 1, 0, "Nm is NULL")
        refused(ptr, 2, 2, 0, "per_instance = 2")
        refused(ptr, 2, 1, 7, "loc = 7")
        for v in (np.nan, np.inf):
            bad = good.copy()
            bad[B - 1, 1, m.nx - 1] = v
            refused(bad.ctypes.data_as(dp), 2, 1, 0, "NaN or infinite")
        for bad_shape in (np.zeros((2, m.nx + 1)), np.zeros((B + 1, 2, m.nx)), np.zeros(m.nx), np.zeros((0, m.nx))):
            with pytest.raises(ValueError, match="meas_noise: the table must be"):
                cl.set_meas_noise(bad_shape)
        with pytest.raises(RuntimeError, match="NaN or infinite"):
            cl.set_meas_noise(np.full((1, m.nx), np.nan))
        # the previous table is still in force: the next slsqp_cl_init latches it
        cl.reset(x0)
        assert np.array_equal(cl.f.get("meas_noise", (2, m.nx)), tab)
        assert np.array_equal(cl.f.get("x_plant", (m.nx,)), x0) and np.array_equal(cl.f.get("x_meas", (m.nx,)), MR.measure(x0, tab, 0))
        # slsqp_set: x_meas writes the measurement only, x_plant the truth only
        y = np.ascontiguousarray(x0 + 0.5)
        assert lib.slsqp_set(h, b"x_meas", y.ctypes.data_as(C.c_void_p), 0) == 0
        assert np.array_equal(cl.f.get("x_plant", (m.nx,)), x0) and np.array_equal(cl.f.get("x_meas", (m.nx,)), y)
        assert lib.slsqp_set(h, b"x_plant", y.ctypes.data_as(C.c_void_p), 0) == 0 and np.array_equal(cl.f.get("x_plant", (m.nx,)), y)
        # a setter call after slsqp_cl_init does not affect the run in progress; the next slsqp_cl_init takes it
        ref, fref = _stepwise(cl, steps, x0, W, **kw)
        other = -2.0 * tab
        L = __import__("robust_nonlinear_mpc_amd")._lib
        L.check(lib.slsqp_cl_log(h, steps))
        cl.reset(x0, **kw)
        for i in range(steps):
            cl.step(W[i], fetch=False)
            if i == 0:
                cl.set_meas_noise(other)
            if i == 1:
                cl.set_meas_noise(None)
                cl.set_meas_noise(other)      # (replacing a table no slsqp_cl_init has latched)
        z = np.zeros((steps, 1))
        got = cl._log_result(steps, z, z, z)
        _same(got, ref, _final(cl), fref, "setter inside a run")
        assert np.array_equal(cl.f.get("meas_noise", (2, m.nx)), tab)
        cl.reset(x0)
        assert np.array_equal(cl.f.get("meas_noise", (2, m.nx)), other) and np.array_equal(cl.f.get("x_meas", (m.nx,)), MR.measure(x0, other, 0))
        # cleared: takes effect at the next slsqp_cl_init too
        cl.set_meas_noise(None)
        assert np.array_equal(cl.f.get("x_plant", (m.nx,)), x0)
        cl.reset(x0)
        assert np.array_equal(cl.f.get("x_meas", (m.nx,)), x0) and np.array_equal(cl.f.get("x_plant", (m.nx,)), x0)
        assert lib.slsqp_result_bytes(h, b"meas_noise") == 0
    finally:
        cl.close()
    bare = types.SimpleNamespace(nx=m.nx, nu=m.nu, nw=m.nw, ni=m.ni, ni_f=m.ni_f, G=m.G, Gf=m.Gf, gf=m.gf, E=m.E)      # (no model_id: the handle gets no plant)
    f = BatchedFastSLS(3, m.Q, m.R, bare, m.Qf, batch=1)
    try:
        with pytest.raises(RuntimeError, match="slsqp_cl_set_meas_noise: handle: slsqp_set_model must be called first"):
            f.set_meas_noise(np.zeros((1, m.nx)))
        assert f.meas_noise is None
    finally:
        f.close()


def test_second_run_on_a_used_handle():
    name, ckw, runner, rkw, _ = ROUTES["k_cl_loop"]
    m, N, B, steps, x0, W, kw = _setup(name)
    tab = _table(m, B)
    cl = _make(m, N, B, tab, **ckw)
    try:
        first, f1 = runner(cl, steps, x0, W, **kw, **rkw)
        cl.set_meas_noise(0.5 * tab[0])
        runner(cl, steps, x0, W, **kw, **rkw)
        cl.set_meas_noise(tab)
        again, f2 = runner(cl, steps, x0, W, **kw, **rkw)
    finally:
        cl.close()
    _same(again, first, f2, f1, "second run", skip=("qp_stats",))      # (step 0's qp_stats of a used handle: tests/test_gpu_hold_persistent.py)
    assert np.array_equal(again["qp_stats"][:, 1:], first["qp_stats"][:, 1:]) and np.array_equal(f2["x_plant"], f1["x_plant"])

"""The state-feedback disturbance adversary of the closed loops (slsqp_cl_set_adversary) on the GPU, at the suite's smallest
shapes (pendulum N = 3, B = 5, 3 steps; rocket N = 4, B = 6, 4 steps; the persistent launches with 2 waves).  Every comparison is np.array_equal.

  1. the rule: w_applied of every instance and step is tests/adversary_ref.py applied to the measured state of that step;
  2. replay: a fresh handle with the option off and W = w_applied gives every shared result key bit for bit, on every route;
  3. routes: under the adversary the persistent launches equal the stepped loop, with plant parameters, bounds, a reference, and all three;
  4. off is off: set and cleared equals never set; an all-zero mask reproduces the plain run; no plant parameters means a model error of zero;
  5. mixing: a mask leaves the other channels at the given W, amp scales the chosen ones, amp > 1 shows in disturbance_used;
  6. refusals, a second run on a used handle, log_w_applied without a log.

Under the adversary a handle without plant parameters runs the PP instantiations of the persistent kernels with the model's own row, which takes the
statements of the kernels without parameters (cl_plant_one): replay, routes and the zero mask compare across that boundary for the rocket's k_cl_loop.
"""
import types

import numpy as np
import pytest

import adversary_ref as AR
import loop_args_runs as R

pytestmark = pytest.mark.gpu

TIMING_KEYS = ("t_jac", "t_qp", "t_riccati", "loop_stats", "rounds")


def _shapes(name):
    return dict(N=3, B=5, steps=3) if name == "pendulum" else dict(N=4, B=6, steps=4)


def _setup(name):
    m, N, B, steps, x0, W, kw = R.setup(name, **_shapes(name))
    if name == "pendulum":
        # x0 / -x0 pairs with every component off zero, and one instance with a zero component (the tie)
        base = np.array([0.5, 0.5, 0.1, -0.1])
        x0 = np.stack([base, -base, 1.05 * base, -1.05 * base, base * np.array([1.0, 1.0, 0.0, 1.0])])
    return m, N, B, steps, x0, W, kw


def _make(m, N, B, adversary=None, amp=1.0, mask=None, tune=None, **kw):
    from robust_nonlinear_mpc_amd import ClosedLoopMPC
    cl = ClosedLoopMPC(m, N, B, **kw)
    for k, v in (tune or {}).items():
        setattr(cl.f.opts, k, v)
    if adversary is not None:
        cl.set_adversary(adversary, amp, mask)
    return cl


def _stepwise(cl, steps, x0, W, **kw):
    return R.stepwise(cl, steps, x0, W, close=False, **kw)


def _decoupled(cl, steps, x0, W, **kw):
    return R.decoupled(cl, steps, x0, W, close=False, **kw)


def _on_device(cl, steps, x0, W, **kw):
    return cl.run_on_device(x0, steps, W, **kw), R.final(cl)


def _host_run(cl, steps, x0, W, **kw):
    kw.pop("continuation", None)
    return cl.run(x0, steps, W, **kw), R.final(cl)


# route: (plant, constructor keywords, runner, run keywords)
ROUTES = {
    "step": ("pendulum", dict(rti=3, fast_sls_rti_steps=2), _stepwise, {}),
    "run": ("pendulum", dict(rti=3, fast_sls_rti_steps=2), _host_run, {}),
    "run_on_device": ("rocket", {}, _on_device, {}),
    "rounds": ("rocket", dict(tune=dict(cl_persistent=0)), _decoupled, {}),
    "k_cl_loop": ("rocket", {}, _decoupled, {}),
    "k_cl_loop_scp": ("pendulum", dict(rti=3, fast_sls_rti_steps=2), _decoupled, {}),
    "sls_converge": ("pendulum", dict(rti=2, fast_sls_rti_steps=None), _decoupled, dict(persistent_converge=True)),
    "solve_every_stepped": ("rocket", {}, _on_device, dict(solve_every=2)),
    "solve_every_persistent": ("rocket", {}, _decoupled, dict(solve_every=2, persistent_hold=True)),
    "plan_fallback": ("rocket", dict(plan_fallback=True), _decoupled, {}),
    "plan_fallback_stepped": ("rocket", dict(plan_fallback=True), _on_device, dict(solve_every=2)),      # (k_cl_plan_fallback + the plant launch, in slsqp_cl_step and slsqp_cl_hold_step)
    "hold_trigger": ("rocket", {}, _decoupled, dict(solve_every=3, persistent_hold=True, hold_trigger=0.5)),
}


def _route(route, W=None, adversary=None, amp=1.0, mask=None, then=None, **opt):
    """One run of a route; `then(cl)` is called on the handle before it is closed.  Returns (out, fin, W, what then returned)."""
    name, ckw, runner, rkw = ROUTES[route]
    m, N, B, steps, x0, W0, kw = _setup(name)
    cl = _make(m, N, B, adversary, amp, mask, **ckw, **opt)
    try:
        out, fin = runner(cl, steps, x0, W0 if W is None else W, **kw, **rkw)
        extra = then(cl) if then else None
    finally:
        cl.close()
    return out, fin, W0, extra


def _differing(x, y):
    """None where the arrays are equal, else (entries that differ, of how many, largest |difference|): the figures an assertion message carries."""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape == y.shape and np.array_equal(x, y, equal_nan=True):
        return None
    if x.shape != y.shape:
        return ("shapes", x.shape, y.shape)
    ne = ~((x == y) | ((x != x) & (y != y)))
    with np.errstate(invalid="ignore"):
        return int(ne.sum()), int(ne.size), float(np.nanmax(np.abs(x.astype(float) - y.astype(float))[ne]))


def _same(a, b, fa=None, fb=None, what="", skip=()):
    keys = [k for k in a if k in b and k not in TIMING_KEYS and k not in skip]
    assert "state_trajectory" in keys and "success" in keys
    bad = {k: d for k in keys for d in [_differing(a[k], b[k])] if d is not None}
    if fa is not None:
        bad.update({"final " + k: d for k in R.FIN_KEYS for d in [_differing(fa[k], fb[k])] if d is not None})
    print(what, "compared", len(keys), "keys; differing:", bad)
    assert not bad, (what, bad)
    return keys


def _expected(m, out, policy, amp, mask, W, bounds=None, Xref=None):
    """adversary_ref on the measured state of every step: (steps, B, nx)"""
    X = out["state_trajectory"]      # (B, nx, steps)
    steps = X.shape[2]
    return np.stack([AR.applied_batch(policy, amp, mask, X[:, :, t], m.E, None if W is None else W[t], s=t, g=m.g, bounds=bounds, Xref=Xref) for t in range(steps)])


# ---- 1: the rule -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["nearest_bound", "away_from_target"])
def test_w_applied_is_the_rule_on_the_measured_state(policy):
    m, N, B, steps, x0, W, kw = _setup("pendulum")
    code = {"nearest_bound": AR.NEAREST_BOUND, "away_from_target": AR.AWAY_FROM_TARGET}[policy]
    # instance 3 has a bounds table of its own that opens the upper side of state 0 to +inf at row 1 (rows 0 and 1; the last row is held)
    g = np.tile(np.asarray(m.g, dtype=float), (B, 2, 1))
    g[3, 1, 0] = np.inf
    # ... and every instance tracks a reference that moves with the step, so policy 2 has something to read
    Xref = np.tile(np.asarray(m.x_ref, dtype=float), (B, 2, 1))
    Xref[:, 1, 0] = 0.45 * np.sign(x0[:, 0])
    cl = _make(m, N, B, policy, 1.0, None, rti=3, fast_sls_rti_steps=2, bounds=(g, None), reference=(Xref, None))
    try:
        out, _ = _stepwise(cl, steps, x0, W, **kw)
        last = cl.f.get("w_applied", (m.nx,))
        assert cl.f.get_adversary() == (code, 1.0)
    finally:
        cl.close()
    wa = out["w_applied"]
    assert wa.shape == (steps, B, m.nx)
    assert np.array_equal(out["state_trajectory"][:, :, 0], x0)
    want = _expected(m, out, code, 1.0, None, W, bounds=g, Xref=Xref[:, :, :m.nx])
    assert np.array_equal(wa, want)
    assert np.array_equal(last, wa[-1])
    # both signs occurred in every channel at step 0, by construction (E is diagonal and positive: x0 / -x0 pairs)
    assert all(m.E[j, j] > 0 for j in range(m.nx))
    assert ((wa[0] == 1.0).any(axis=0) & (wa[0] == -1.0).any(axis=0)).all()
    assert np.isin(wa, (1.0, -1.0)).all()
    if code == AR.NEAREST_BOUND:
        assert wa[0, 4, 2] == 1.0      # the tie: x = 0 in a symmetric box
        assert (wa[1:, 3, 0] == -1.0).all() and wa[0, 3, 0] == -1.0      # (instance 3 starts at -1.05 base; from row 1 on only the lower side is left)
    assert np.array_equal(out["disturbance_used"], np.ones((steps, B)))


# ---- 2: replay ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_replay_with_the_option_off_gives_the_same_bits(route):
    name = ROUTES[route][0]
    m = _setup(name)[0]

    def merr(cl):
        steps = _shapes(name)["steps"]
        return cl.f.get("model_err", (m.nx,)), (cl.f.get("log_model_error", (steps, m.nx)) if route != "run" else None)
    adv, fadv, W, (me, lme) = _route(route, adversary="nearest_bound", then=merr)
    assert "w_applied" in adv and "disturbance_used" in adv and "model_error" not in adv
    wa = adv["w_applied"]
    assert np.array_equal(wa, _expected(m, adv, AR.NEAREST_BOUND, 1.0, None, W))
    assert not me.any() and (lme is None or not lme.any())      # no plant parameters: the model's step, a model error of exactly zero
    rep, frep, _, _ = _route(route, W=wa)
    assert "w_applied" not in rep and "disturbance_used" not in rep
    _same(adv, rep, fadv, frep, route)


@pytest.mark.parametrize("route", ["k_cl_loop", "solve_every_persistent", "plan_fallback", "hold_trigger"])
def test_replay_and_zero_mask_against_the_models_own_row(route):
    """The replay and the all-zero mask of the rocket's persistent routes once more, with the handle that has the option off given the model's plant
    parameters explicitly: both sides then launch the same instantiation of k_cl_loop (the PP variants, whose `is_model` rule takes the model's step),
    so what is compared is the option alone."""
    from robust_nonlinear_mpc_amd import plant_param_defaults
    m = _setup("rocket")[0]
    d = plant_param_defaults(m)
    adv, fadv, W, _ = _route(route, adversary="nearest_bound")
    rep, frep, _, _ = _route(route, W=adv["w_applied"], plant_params=d)
    assert "w_applied" not in rep and not rep["model_error"].any()
    _same(adv, rep, fadv, frep, (route, "replay"))
    zero, fzero, _, _ = _route(route, adversary="nearest_bound", mask=np.zeros(m.nx))
    plain, fplain, _, _ = _route(route, plant_params=d)
    assert np.array_equal(zero["w_applied"], W)
    _same(zero, plain, fzero, fplain, (route, "zero mask"))


# ---- 3: routes ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pendulum", "rocket"])
@pytest.mark.parametrize("state", [(0, 1, 0), (0, 0, 1), (1, 0, 0), (1, 1, 1)], ids=["params", "bounds", "reference", "all"])
def test_persistent_launch_equals_the_stepped_loop_under_the_adversary(name, state):
    m, N, B, steps, x0, W, kw = _setup(name)
    mk = R.option_state(m, B, state)
    ckw = dict(rti=3, fast_sls_rti_steps=2) if name == "pendulum" else {}
    policy = "away_from_target" if state == (1, 0, 0) else "nearest_bound"
    outs = []
    for runner in (_stepwise, _decoupled):
        cl = _make(m, N, B, policy, 1.0, None, **ckw, **mk)
        try:
            outs.append(runner(cl, steps, x0, W, **kw))
        finally:
            cl.close()
    (a, fa), (b, fb) = outs
    keys = _same(a, b, fa, fb, (name, state))
    assert "w_applied" in keys and "disturbance_used" in keys and ("model_error" in keys) == bool(state[1]) and ("constraint_margin" in keys) == bool(state[2])
    code = AR.AWAY_FROM_TARGET if state == (1, 0, 0) else AR.NEAREST_BOUND
    want = _expected(m, a, code, 1.0, None, W, bounds=mk["bounds"][0] if state[2] else None, Xref=mk["reference"][0] if state[0] else None)
    assert np.array_equal(a["w_applied"], want)
    if state[1]:
        assert a["model_error"].any()      # parameters off their defaults: the plant's own step


# ---- 4: off is off -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_off_is_off(route):
    plain, fplain, W, _ = _route(route)
    assert "w_applied" not in plain
    name, ckw, runner, rkw = ROUTES[route]
    m, N, B, steps, x0, _, kw = _setup(name)
    # set and cleared: a handle that never had it
    cl = _make(m, N, B, "away_from_target", 0.7, None, **ckw)
    try:
        cl.set_adversary(None)
        assert cl.f.get_adversary()[0] == 0
        out, fin = runner(cl, steps, x0, W, **kw, **rkw)
    finally:
        cl.close()
    assert "w_applied" not in out
    _same(out, plain, fin, fplain, (route, "cleared"))
    # a run under the adversary, then cleared on the same handle: the block of the persistent launches says "off" again
    cl = _make(m, N, B, "nearest_bound", 1.0, None, **ckw)
    try:
        runner(cl, steps, x0, W, **kw, **rkw)
        cl.set_adversary("off")
        out, fin = runner(cl, steps, x0, W, **kw, **rkw)
    finally:
        cl.close()
    _same(out, plain, fin, fplain, (route, "run, then cleared"), skip=("qp_stats",))      # (step 0's qp_stats of a used handle: tests/test_gpu_hold_persistent.py)
    # an all-zero mask: every channel keeps the given W
    zero, fzero, _, _ = _route(route, adversary="nearest_bound", mask=np.zeros(m.nx))
    assert np.array_equal(zero["w_applied"], W)
    _same(zero, plain, fzero, fplain, (route, "zero mask"))


# ---- 5: mixing ---------------------------------------------------------------------------------------------------------------------------------------
def test_mask_amp_and_disturbance_used():
    route = "k_cl_loop"
    m = _setup("rocket")[0]
    mask = np.zeros(m.nx)
    mask[[1, 13]] = 1
    full, _, W, _ = _route(route, adversary="nearest_bound", amp=1.0, mask=mask)
    wa = full["w_applied"]
    off_mask = mask == 0
    assert np.array_equal(wa[:, :, off_mask], W[:, :, off_mask])      # the others stay at the given W
    assert np.isin(wa[:, :, ~off_mask], (1.0, -1.0)).all()
    assert np.array_equal(wa, _expected(m, full, AR.NEAREST_BOUND, 1.0, mask, W))
    half, _, _, _ = _route(route, adversary="nearest_bound", amp=0.5, mask=mask)
    wh = half["w_applied"]
    assert np.array_equal(wh[0], np.where(off_mask[None, :], W[0], 0.5 * wa[0]))      # step 0 starts from the same state: the same signs, halved
    assert np.isin(wh[:, :, ~off_mask], (0.5, -0.5)).all() and np.array_equal(wh[:, :, off_mask], W[:, :, off_mask])
    big, _, _, _ = _route(route, adversary="nearest_bound", amp=1.5, mask=mask)
    assert np.array_equal(big["disturbance_used"], np.full(big["disturbance_used"].shape, 1.5))
    assert (full["disturbance_used"] <= 1.0).all()


# ---- 6: refusals and plumbing ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from robust_nonlinear_mpc_amd import BatchedFastSLS
    m, N, B, steps, x0, W, kw = _setup("pendulum")
    cl = _make(m, N, B, rti=3, fast_sls_rti_steps=2)
    lib, h = cl.f.lib, cl.f.h
    cl.set_adversary("nearest_bound", 0.75, [1, 0, 1, 0])
    assert cl.f.get_adversary() == (1, 0.75)

    def refused(policy, amp, words):
        assert lib.slsqp_cl_set_adversary(h, policy, amp, None) != 0
        assert words in lib.slsqp_last_error().decode()
        assert cl.f.get_adversary() == (1, 0.75)      # the previous setting stays in force
    refused(3, 1.0, "policy = 3")
    refused(-1, 1.0, "policy = -1")
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        refused(2, bad, "amp = ")
    for bad in ("closest", 7, True):
        with pytest.raises(ValueError, match="unknown policy"):
            cl.set_adversary(bad)
    with pytest.raises(ValueError, match="amp must be finite"):
        cl.set_adversary("nearest_bound", -2.0)
    with pytest.raises(ValueError, match="mask must be"):
        cl.set_adversary("nearest_bound", 1.0, [1, 0])
    assert cl.f.get_adversary() == (1, 0.75)
    assert lib.slsqp_cl_set_adversary(h, 2, 1.5, None) == 0 and cl.f.get_adversary() == (2, 1.5)      # amp > 1 is accepted
    # log_w_applied without a log
    with pytest.raises(RuntimeError, match="unknown result name: log_w_applied"):
        cl.f.get("log_w_applied", (steps, m.nx))
    assert not cl.f.get("w_applied", (m.nx,)).any()      # no plant step yet
    cl.close()
    # a general G (such a handle never gets a model: slsqp_set_model refuses it)
    gen = types.SimpleNamespace(nx=m.nx, nu=m.nu, nw=m.nw, ni=m.ni, ni_f=m.ni_f, G=2.0 * np.asarray(m.G), Gf=m.Gf, gf=m.gf, E=m.E)
    f = BatchedFastSLS(3, m.Q, m.R, gen, m.Qf, batch=1)
    try:
        assert f.lib.slsqp_cl_set_adversary(f.h, 2, 1.0, None) != 0 and "slsqp_cl_set_adversary: handle: general G" in f.lib.slsqp_last_error().decode()
        with pytest.raises(RuntimeError, match="slsqp_cl_set_adversary: handle: general G"):
            f.set_adversary("away_from_target")
        assert f.adversary is None and f.get_adversary()[0] == 0
    finally:
        f.close()
    # a handle without slsqp_set_model
    bare = types.SimpleNamespace(nx=m.nx, nu=m.nu, nw=m.nw, ni=m.ni, ni_f=m.ni_f, G=m.G, Gf=m.Gf, gf=m.gf, E=m.E)      # (no model_id: the handle gets no plant)
    f = BatchedFastSLS(3, m.Q, m.R, bare, m.Qf, batch=1)
    try:
        assert f.lib.slsqp_cl_set_adversary(f.h, 1, 1.0, None) != 0 and "slsqp_set_model must be called first" in f.lib.slsqp_last_error().decode()
        with pytest.raises(RuntimeError, match="slsqp_cl_set_adversary: handle: slsqp_set_model must be called first"):
            f.set_adversary("nearest_bound")
        assert f.adversary is None and f.get_adversary()[0] == 0
    finally:
        f.close()


def test_second_run_on_a_used_handle():
    name, ckw, runner, rkw = ROUTES["k_cl_loop"]
    m, N, B, steps, x0, W, kw = _setup(name)
    cl = _make(m, N, B, "nearest_bound", 1.0, None, **ckw)
    try:
        first, f1 = runner(cl, steps, x0, W, **kw, **rkw)
        cl.set_adversary("away_from_target", 0.5)
        runner(cl, steps, x0, W, **kw, **rkw)
        cl.set_adversary("nearest_bound", 1.0)
        again, f2 = runner(cl, steps, x0, W, **kw, **rkw)
    finally:
        cl.close()
    _same(again, first, f2, f1, "second run", skip=("qp_stats",))      # (step 0's qp_stats of a used handle: tests/test_gpu_hold_persistent.py)
    assert np.array_equal(again["qp_stats"][:, 1:], first["qp_stats"][:, 1:])

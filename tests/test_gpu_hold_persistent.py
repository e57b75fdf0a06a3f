"""Hold steps inside the persistent closed-loop launch (slsqp_cl_set_solve_every, k_cl_loop's HOLD variants).

Every comparison is np.array_equal over every key two results share except the t_* timings: the persistent launch against
run_on_device(x0, steps, W, solve_every=M) on a fresh handle with the same data -- one slsqp_cl_step or slsqp_cl_hold_step per step for the whole
batch, the path tests/test_gpu_hold.py holds against the numpy restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import bounds_cases as BC
import plant_params_helpers as H
import reference_cases as RC

pytestmark = pytest.mark.gpu


def _lib():
    return __import__("robust_nonlinear_mpc_amd")._lib


def _make(m, N, B, rti=None, rti_steps=None, **kw):
    from robust_nonlinear_mpc_amd import ClosedLoopMPC
    return ClosedLoopMPC(m, N, B, rti=rti, fast_sls_rti_steps=rti_steps, **kw)


def _x0(m, B, scale=0.3):
    """Per-instance initial states around the script's (pendulum, rocket) or near the neutral point (quadrotor), as tests/test_gpu_hold.py."""
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


def _final(cl):
    m, N, f = cl.m, cl.N, cl.f
    return dict(x_meas=f.get("x_meas", (m.nx,)), nominal_x=f.get("nominal_x", (N + 1, m.nx)), nominal_u=f.get("nominal_u", (N, m.nu)), u0=f.get("u0", (m.nu,)),
                hold_xi=f.get("hold_xi", (N + 1, m.nx)), hold_index=f.get("hold_index", (), np.int32), hold_policy=f.get("hold_policy", (), np.int32))


def _same(a, b, skip=()):
    shared = [k for k in a if k in b and not k.startswith("t_") and k not in skip]
    assert shared
    for k in shared:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _same_rerun(a, b):
    """A second run on a handle against a fresh handle: every shared key, except that the qp_stats of step 0 are compared in their status only.  The
    first QP of a used handle finds the previous run's warm data, so the statistics of the path it took (not its certified answer) may differ from a
    fresh handle's; that is so for M = 1 on the untouched kernel as well, and from step 1 on the statistics are equal again."""
    _same(a, b, skip=("loop_stats", "qp_stats"))
    assert np.array_equal(a["qp_stats"][:, 1:], b["qp_stats"][:, 1:]) and np.array_equal(a["qp_stats"][:, 0, :, 6], b["qp_stats"][:, 0, :, 6])


def _stepped(m, N, B, M, steps, x0, W, rti=None, rti_steps=None, **kw):
    """The parent's path on a fresh handle: result, final state."""
    cl = _make(m, N, B, rti, rti_steps, **kw)
    out = cl.run_on_device(x0, steps, W, solve_every=M)
    fin = _final(cl)
    cl.close()
    return out, fin


def _persistent(m, N, B, M, steps, x0, W, rti=None, rti_steps=None, waves=None, cl=None, **kw):
    """The persistent launch with hold steps: result, final state (the handle is closed unless it was passed in)."""
    own = cl is None
    if own:
        cl = _make(m, N, B, rti, rti_steps, **kw)
    if waves is not None:
        os.environ["SLSQP_LOOP_WAVES"] = str(waves)
    try:
        out = cl.run_decoupled(x0, steps, W, solve_every=M, persistent_hold=True)
    finally:
        os.environ.pop("SLSQP_LOOP_WAVES", None)
    fin = _final(cl)
    if own:
        cl.close()
    return out, fin


def _check_hold_run(out, fin, ref, ref_fin, B, M, steps):
    _same(out, ref)
    _same(fin, ref_fin)
    assert set(fin) == set(ref_fin)
    assert np.array_equal(out["hold_index"], np.tile(np.arange(steps) % M, (B, 1))) and out["hold_policy"].any()
    assert (fin["hold_index"] == (steps - 1) % M).all()
    assert out["rounds"] == 1 and out["loop_stats"]["mpc_steps"] == B * steps
    hold_at = np.arange(steps) % M != 0
    qs = out["qp_stats"]
    assert qs.shape == (B, steps, 2, 8)
    assert (qs[:, hold_at][..., 6] == -1).all() and not np.delete(qs[:, hold_at], 6, axis=-1).any()      # "took no part" in both slots, 0 everywhere else
    assert (qs[:, ~hold_at, 0, 6] != -1).all()      # a solved step ran its first QP
    assert not out["x0_violation"][:, hold_at].any() and not out["scp_iterations"][:, hold_at].any()


# ---- 1: the main cases ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,rti,rti_steps,N,B,M,steps,waves", [
    ("rocket", 1, 1, 4, 3, 4, 6, None),        # the hold index reaches N - 1; two solves
    ("pendulum", 1, 1, 4, 5, 3, 7, None),
    ("quadrotor", 1, 1, 3, 3, 2, 4, None),     # the (13, 4) code path
    ("rocket", 1, 1, 4, 70, 2, 5, 7),          # 70 instances on 7 waves: instances queue up and change waves
])
def test_persistent_hold_is_the_stepped_loop_bit_for_bit(model, rti, rti_steps, N, B, M, steps, waves):
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    ref, ref_fin = _stepped(m, N, B, M, steps, x0, W, rti, rti_steps)
    out, fin = _persistent(m, N, B, M, steps, x0, W, rti, rti_steps, waves=waves)
    _check_hold_run(out, fin, ref, ref_fin, B, M, steps)
    assert out["loop_stats"]["waves"] == (B if waves is None else waves)
    assert ref["success"].any() and np.abs(fin["hold_xi"]).max() > 0      # the columns of the last hold step


# ---- 2: the four new variants -----------------------------------------------------------------------------------------------------------------------
def _rocket_options(m, B, T):
    refs = [RC.figure8(m, T, z) for z in 0.05 * np.arange(B)]
    reference = (np.stack([m.x_ref + 0.2 * (r[0] - m.x_ref) for r in refs]), np.stack([r[1] for r in refs]))
    P = H.spread_params(m, B, 10.0, seed=5)
    bounds = BC._rows(m, T, {m.nx + j: (None, BC._from(T, 1, 0.9 * m.u_ub[j], np.inf)) for j in range(m.nu)})
    return reference, P, bounds


@pytest.mark.parametrize("which", ["ref", "pp", "bnd", "all"])
def test_every_hold_variant_of_the_kernel(which):
    """k_cl_loop<rocket, 9 | 11 | 13 | 15>: a reference only, then plant parameters, then bounds, then all three."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("rocket")
    N, B, M, steps = 4, 3, 2, 4
    reference, P, bounds = _rocket_options(m, B, steps + N + 1)
    kw = {}
    if which in ("ref", "all"):
        kw["reference"] = reference
    if which in ("pp", "all"):
        kw["plant_params"] = P
    if which in ("bnd", "all"):
        kw["bounds"] = bounds
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    ref, ref_fin = _stepped(m, N, B, M, steps, x0, W, 1, 1, **kw)
    out, fin = _persistent(m, N, B, M, steps, x0, W, 1, 1, **kw)
    _check_hold_run(out, fin, ref, ref_fin, B, M, steps)
    if which != "bnd":      # the option reaches the run (bounds that no input touches need not move a bit; their margin below says they are set)
        plain, _ = _stepped(m, N, B, M, steps, x0, W, 1, 1)
        assert not np.array_equal(plain["state_trajectory"], ref["state_trajectory"])
    if "plant_params" in kw:
        hold_at = np.arange(steps) % M != 0
        assert np.array_equal(out["model_error"][:, :, hold_at], ref["model_error"][:, :, hold_at]) and np.abs(out["model_error"][:, :, hold_at]).max() > 1e-9
    if "bounds" in kw:
        assert np.array_equal(out["constraint_margin"], ref["constraint_margin"])


# ---- 3: an instance without a valid plan ------------------------------------------------------------------------------------------------------------
def test_refused_instance_applies_the_nominal_input_and_the_others_do_not_notice():
    """Row 0 of instance 1's bounds puts the upper bound of its cart position 1e-3 below its measured state (the device of
    tests/test_gpu_hold.py::test_failed_instance_applies_the_nominal_input_and_the_others_do_not_notice, at the run's first step: row 0 is stage 0
    of step 0's window and of no other): under the strict gate its first solve is refused, the hold step that follows gives it the shifted nominal
    input and hold_policy = 0; the other instances have the bits of a batch without the offset."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("pendulum")
    N, B, M, steps = 6, 4, 2, 4
    x0 = np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.1 * np.arange(B)[:, None])
    W = _seeded_W(m, B, steps)
    g = np.tile(m.g, (B, steps + N + 1, 1))
    gf = np.tile(m.gf, (B, steps + N + 1, 1))
    ref, ref_fin = _persistent(m, N, B, M, steps, x0, W, 1, 1, bounds=(g.copy(), gf))
    g[1, 0, 0] = x0[1, 0] - 1e-3
    out, fin = _persistent(m, N, B, M, steps, x0, W, 1, 1, bounds=(g, gf))
    stepped, stepped_fin = _stepped(m, N, B, M, steps, x0, W, 1, 1, bounds=(g, gf))
    _same(out, stepped)
    _same(fin, stepped_fin)
    assert ref["success"][:, 0].all() and not out["success"][1, 0] and out["success"][[0, 2, 3], 0].all()
    assert ref["hold_policy"][:, 1].all() and list(out["hold_policy"][:, 1]) == [True, False, True, True]
    assert np.array_equal(out["input_trajectory"][1, :, 1], out["nominal_trajectory_u"][1, :, 0, 1])      # the shifted nominal input
    assert not np.array_equal(ref["input_trajectory"][1, :, 1], ref["nominal_trajectory_u"][1, :, 0, 1])
    others = [0, 2, 3]
    for k in out:
        if isinstance(out[k], np.ndarray) and out[k].ndim >= 2 and out[k].shape[0] == B and not k.startswith(("t_", "bounds_")) and k != "constraint_margin":      # (steps, B)
            assert np.array_equal(out[k][others], ref[k][others], equal_nan=True), k
    for k in fin:
        assert np.array_equal(fin[k][others], ref_fin[k][others]), k


# ---- 4: qp_stats ------------------------------------------------------------------------------------------------------------------------------------
def test_qp_stats_of_solved_steps_are_the_stepped_solves():
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("rocket")
    N, B, M, steps = 4, 3, 2, 5
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    cl = _make(m, N, B, 1, 1)
    cl.reset(x0)
    stats = {}
    for i in range(steps):
        if i % M:
            cl.hold_step(W[i], fetch=False)
        else:
            cl.step(W[i], fetch=False)
            stats[i] = cl.f.get("qp_stats", (2, 8), np.int32)
    cl.close()
    out, _ = _persistent(m, N, B, M, steps, x0, W, 1, 1)
    for i in range(steps):
        if i in stats:
            assert np.array_equal(out["qp_stats"][:, i], stats[i]), i
        else:
            assert (out["qp_stats"][:, i, :, 6] == -1).all() and not np.delete(out["qp_stats"][:, i], 6, axis=-1).any(), i


# ---- 5: M = 1, reruns -------------------------------------------------------------------------------------------------------------------------------
def test_solve_every_one_launches_todays_loop():
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("rocket")
    N, B, steps = 4, 3, 4
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    a = _make(m, N, B, 1, 1)
    plain = a.run_decoupled(x0, steps, W)
    plain_fin = _final(a)
    a.close()
    b = _make(m, N, B, 1, 1)
    b.f.set_solve_every(1)
    assert b.f.get_solve_every() == 1
    one = b.run_decoupled(x0, steps, W)
    one_fin = _final(b)
    b.close()
    c = _make(m, N, B, 1, 1)
    hold1 = c.run_decoupled(x0, steps, W, solve_every=1, persistent_hold=True)      # M = 1 with the flag: nothing to hold
    c.close()
    assert plain["loop_stats"]["mpc_steps"] == B * steps and one["loop_stats"]["mpc_steps"] == B * steps
    assert set(one) == set(plain) and "hold_index" not in one and set(hold1) == set(plain)
    _same(one, plain, skip=("loop_stats",))
    _same(hold1, plain, skip=("loop_stats",))
    _same(one_fin, plain_fin)
    assert not one_fin["hold_index"].any() and not one_fin["hold_xi"].any()


def test_reruns_on_one_handle_give_the_bits_of_fresh_handles():
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("rocket")
    N, B, M, steps = 4, 3, 2, 5
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    fresh, fresh_fin = _persistent(m, N, B, M, steps, x0, W, 1, 1)
    a = _make(m, N, B, 1, 1)
    plain = a.run_decoupled(x0, steps, W)
    a.close()
    cl = _make(m, N, B, 1, 1)
    for _ in range(2):      # the same handle twice: the second run starts from whatever the first left in the hold state, the block and the log
        out, fin = _persistent(m, N, B, M, steps, x0, W, cl=cl)
        _same_rerun(out, fresh)
        _same(fin, fresh_fin)
    again = cl.run_decoupled(x0, steps, W)      # M = 1 after M = 2
    assert cl.f.get_solve_every() == 1 and "hold_index" not in again
    _same_rerun(again, plain)
    assert not cl.f.get("hold_index", (), np.int32).any()
    with pytest.raises(RuntimeError, match="leave no per-batch plan"):      # as after every persistent run
        cl.f.hold_step(None)
    cl.close()


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from robust_nonlinear_mpc_amd import get_model
    L = _lib()
    m = get_model("rocket")
    N, B, steps = 4, 3, 3
    x0, W = _x0(m, B), np.ascontiguousarray(_seeded_W(m, B, steps))
    cl = _make(m, N, B, 1, 1)
    cl.reset(x0)

    def state(c):
        return [c.f.get(k, s) for k, s in (("x_meas", (c.m.nx,)), ("nominal_x", (c.N + 1, c.m.nx)), ("nominal_u", (c.N, c.m.nu)))] + [np.array(c.f.get_solve_every())]

    def refused(c, word, call):
        before = state(c)
        with pytest.raises(RuntimeError, match=word):
            call()
        assert all(np.array_equal(a, b) for a, b in zip(before, state(c)))

    refused(cl, "outside 1 .. N", lambda: cl.f.set_solve_every(0))
    refused(cl, "outside 1 .. N", lambda: cl.f.set_solve_every(N + 1))
    cl.f.set_solve_every(2)
    wp = W.ctypes.data_as(C.c_void_p)
    cl.f.opts.cl_persistent = 0
    refused(cl, "persistent launch only", lambda: L.check(cl.f.lib.slsqp_cl_run(cl.f.h, steps, wp, L.HOST, C.byref(cl.f.opts), 8.0, 0.0, None)))
    cl.f.opts.cl_persistent = 1
    refused(cl, "needs rti = 1 with one fast-SLS step", lambda: L.check(cl.f.lib.slsqp_cl_run_scp(cl.f.h, steps, 3, wp, L.HOST, C.byref(cl.f.opts))))
    cl.f.set_solve_every(1)
    # the handle still runs, and gives the bits of a fresh one
    out, fin = _persistent(m, N, B, 2, steps, x0, W, cl=cl)
    cl.close()
    fresh, fresh_fin = _persistent(m, N, B, 2, steps, x0, W, 1, 1)
    _same(out, fresh, skip=("loop_stats",))      # (no run before it on this handle: the qp_stats too)
    _same(fin, fresh_fin)
    # the pendulum's script setting (rti = 3, two fast-SLS steps) has no hold inside its persistent kernel
    mp = get_model("pendulum")
    cp = _make(mp, 4, 3)
    cp.reset(_x0(mp, 3))
    refused(cp, "needs rti = 1 with one fast-SLS step", lambda: cp.run_decoupled(1.1 * _x0(mp, 3), 4, None, solve_every=2, persistent_hold=True))
    stepped = cp.run_decoupled(_x0(mp, 3), 4, None, solve_every=2)      # the default: Python steps the loop, as before
    assert stepped["rounds"] == 4 and "qp_stats" not in stepped
    cp.close()


# ---- 7: the Monte-Carlo driver ----------------------------------------------------------------------------------------------------------------------
def test_monte_carlo_persistent_hold_equals_the_default_path():
    from robust_nonlinear_mpc_amd import get_model, run_monte_carlo
    m = get_model("rocket")
    N, S, steps, M = 4, 5, 4, 2
    x0 = m.x_ref + 0.3 * (m.extra["x0"] - m.x_ref)
    default = run_monte_carlo(m, N, np.arange(S), steps, x0, slices=2, solve_every=M)
    pers = run_monte_carlo(m, N, np.arange(S), steps, x0, slices=2, solve_every=M, persistent=True)
    assert "qp_stats" not in default and "loop_stats" not in default
    assert pers["qp_stats"].shape == (S, steps, 2, 8) and pers["rounds"] == [1, 1] and sum(s["mpc_steps"] for s in pers["loop_stats"]) == S * steps
    _same(pers, default)
    assert np.array_equal(pers["hold_index"], np.tile(np.arange(steps) % M, (S, 1))) and pers["hold_policy"].any()

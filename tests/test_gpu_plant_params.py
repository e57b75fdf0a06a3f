"""Plant parameter mismatch in the on-device closed loops (slsqp_cl_set_plant_params): the plant step against the host's ddyn_p, the controller
untouched, explicit defaults = nothing set = set and cleared, the persistent loops bit for bit the step-by-step loop, shared = equal rows, the CPU
oracle loop with the mismatched plant, the Monte-Carlo driver's cut, the refusals, and the setter under debug allocators."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import plant_params_helpers as H
from conftest import ROOT

pytestmark = pytest.mark.gpu

LOG_KEYS = ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x", "backoff_trajectory_u", "success",
            "scp_iterations", "primal_infeasibility", "x0_violation")
PP_KEYS = ("model_error", "disturbance_used")


def _final(cl):
    m, N = cl.m, cl.N
    return {k: cl.f.get(k, shp) for k, shp in (("x_meas", (m.nx,)), ("nominal_x", (N + 1, m.nx)), ("nominal_u", (N, m.nu)), ("primal_vec", (cl.f.n,)),
                                               ("model_err", (m.nx,)))}


def _make(m, N, B, rti=None, rti_steps=None, reference=None, tune=None, plant_params=None):
    from robust_nonlinear_mpc_amd import ClosedLoopMPC
    cl = ClosedLoopMPC(m, N, B, rti=rti, fast_sls_rti_steps=rti_steps, reference=reference, plant_params=plant_params)
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
    out["log_model_error"] = cl.f.get("log_model_error", (steps, cl.m.nx))
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
    out["log_model_error"] = cl.f.get("log_model_error", (steps, cl.m.nx))
    fin = _final(cl)
    cl.close()
    return out, fin


def _assert_same(out, fin, ref, ref_fin, what="", keys=LOG_KEYS + ("qp_stats", "log_model_error")):
    for k in keys:
        assert np.array_equal(out[k], ref[k], equal_nan=True), (what, k)
    for k in fin:
        assert np.array_equal(fin[k], ref_fin[k], equal_nan=True), (what, k)


def _seeded_W(m, B, steps):
    from robust_nonlinear_mpc_amd import disturbance_stream
    return np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)


def _wavy_reference(m, B, T, amp):
    Xref = np.tile(np.asarray(m.x_ref, dtype=float), (B, T, 1))
    t, b = np.arange(T)[None, :], np.arange(B)[:, None]
    for i in range(min(3, m.nx)):
        Xref[:, :, i] += amp * np.sin(0.35 * t + 0.7 * b + i)
    return Xref, np.tile(np.asarray(m.u_ref, dtype=float), (B, T, 1))


def _x0(m, B, scale=0.3):
    """Per-instance initial states around the script's (pendulum, rocket) or near the neutral point (quadrotor)."""
    rng = np.random.default_rng(21)
    if m.name == "quadrotor":
        x0 = m.x_ref + 0.02 * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, (B, m.nx))
        x0[:, 6:10] /= np.linalg.norm(x0[:, 6:10], axis=1, keepdims=True)
        return x0
    s = scale if m.name == "rocket" else 1.0
    return m.x_ref + s * (m.extra["x0"] - m.x_ref) * (1.0 + 0.1 * rng.uniform(-1, 1, (B, 1)))


# ---- 1: one step ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,B", [("pendulum", 10, 5), ("quadrotor", 8, 5), ("rocket", 5, 3)])
def test_one_step_plant_is_host_ddyn_p_and_controller_is_untouched(model, N, B):
    """x_meas+ = ddyn_p(x, u0) + E w and model_err = ddyn_p - ddyn against the host instantiation of csrc/dynamics.hpp (pinned to the reference by
    tests/test_plant_params_cpu.py) to 1e-12, u0 from the log; every controller output of the step has the bits of a handle without parameters."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    P = H.spread_params(m, B, 20.0, seed=5)
    x0, W = _x0(m, B), _seeded_W(m, B, 1)
    got = {}
    names = (("u0", (m.nu,)), ("nominal_x", (N + 1, m.nx)), ("nominal_u", (N, m.nu)), ("backoff_x", (N + 1, m.nx)), ("backoff_u", (N, m.nu)),
             ("backoff", (N, m.ni)), ("backoff_f", (m.ni_f,)), ("primal_vec", (m.n_var(N),)), ("dual_vec", (N * (m.nx + m.ni) + m.ni_f,)), ("x_meas", (m.nx,)), ("model_err", (m.nx,)))
    for kind in ("plain", "pp"):
        cl = _make(m, N, B, plant_params=P if kind == "pp" else None)
        L = __import__("robust_nonlinear_mpc_amd")._lib
        L.check(cl.f.lib.slsqp_cl_log(cl.f.h, 1))
        cl.reset(x0)
        cl.step(W[0], fetch=False)
        got[kind] = {k: cl.f.get(k, s) for k, s in names}
        got[kind]["log_u0"] = cl.f.get("log_u0", (1, m.nu))[:, 0]
        got[kind]["log_model_error"] = cl.f.get("log_model_error", (1, m.nx))[:, 0]
        got[kind]["success"] = cl.f.get("scp_success", (), np.int32)
        got[kind]["plant_params"] = cl.f.get("plant_params", (P.shape[1],))
        cl.close()
    g, p = got["pp"], got["plain"]
    assert np.array_equal(g["plant_params"], P) and np.array_equal(p["plant_params"], np.tile(H.host_defaults(m.model_id), (B, 1)))
    for k in ("u0", "nominal_x", "nominal_u", "backoff_x", "backoff_u", "backoff", "backoff_f", "primal_vec", "dual_vec", "log_u0", "success"):
        assert np.array_equal(g[k], p[k], equal_nan=True), k
    assert np.array_equal(g["log_u0"], g["u0"]) and np.array_equal(g["log_model_error"], g["model_err"])
    assert not p["model_err"].any() and not p["log_model_error"].any()
    for b in range(B):
        fp, fc = H.host_ddyn_p(m.model_id, x0[b], g["log_u0"][b], P[b]), H.host_ddyn_c(m.model_id, x0[b], g["log_u0"][b])
        e_x = np.abs(g["x_meas"][b] - (fp + m.E @ W[0][b])).max()
        e_m = np.abs(g["model_err"][b] - (fp - fc)).max()
        print(model, b, "x_meas err", e_x, "model_err err", e_m, "|model_err|", np.abs(fp - fc).max())
        assert e_x < 1e-12 and e_m < 1e-12, (b, e_x, e_m)
        assert np.abs(fp - fc).max() > 1e-6, b      # the parameters reach the step
        assert np.abs(p["x_meas"][b] - (fc + m.E @ W[0][b])).max() < 1e-12, b


# ---- 2: defaults ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["pendulum", "rocket"])
def test_explicit_defaults_nothing_set_and_cleared_are_the_same_bits(model):
    """3 steps, step by step and persistent: a handle that never saw parameters, one with the defaults set explicitly (shared and per instance) and
    one whose parameters were set and cleared give identical result arrays; with explicit defaults log_model_error is exactly zero."""
    from robust_nonlinear_mpc_amd import get_model, plant_param_defaults
    m = get_model(model)
    if model == "pendulum":
        N, B, steps, rti, rti_steps, W, kw = 10, 4, 3, None, None, None, {}
    else:
        N, B, steps, rti, rti_steps, kw = 20, 4, 3, 1, 1, dict(solve_nominal=True, continuation=2)
        W = _seeded_W(m, B, steps)
    x0 = _x0(m, B)
    d = plant_param_defaults(m)

    def handle(kind):
        cl = _make(m, N, B, rti, rti_steps)
        if kind == "defaults":
            cl.set_plant_params(d)
        elif kind == "defaults_rows":
            cl.set_plant_params(np.tile(d, (B, 1)))
        elif kind == "cleared":
            cl.set_plant_params(H.spread_params(m, B, 10.0, seed=1))
            cl.set_plant_params(None)
        return cl
    for run in (_stepwise, _decoupled):
        ref, ref_fin = run(handle("never"), steps, x0, W, **kw)
        assert ref["success"].any() and not ref["log_model_error"].any()
        for kind in ("defaults", "defaults_rows", "cleared"):
            out, fin = run(handle(kind), steps, x0, W, **kw)
            _assert_same(out, fin, ref, ref_fin, (run.__name__, kind))
            if kind != "cleared":
                assert not out["model_error"].any() and np.array_equal(out["disturbance_used"], np.max(np.abs(W), axis=2) if W is not None else np.zeros((steps, B)))


# ---- 3: persistent = step by step -----------------------------------------------------------------------------------------------------------
def _tune_converge(o):
    o.scp_eps = 1e-8


@pytest.mark.parametrize("with_reference", [False, True])
@pytest.mark.parametrize("model,N,B,steps,waves,rti,rti_steps,tune", [
    ("rocket", 20, 96, 4, 7, 1, 1, None),
    ("pendulum", 10, 50, 6, 7, None, None, None),
    ("pendulum", 10, 8, 2, None, -1, 2, _tune_converge),
])
def test_persistent_loops_are_bitwise_the_step_by_step_loop_with_plant_params(model, N, B, steps, waves, rti, rti_steps, tune, with_reference):
    """As test_persistent_loops_are_bitwise_the_step_by_step_loop_with_a_reference (tests/test_gpu_reference.py): with 7 waves for 96 or 50 instances
    the instances are at different steps at the same time and change hands, so every plant step must read its own instance's row.  Rocket: rti 1 /
    one fast-SLS step (k_cl_loop<M, 3>, VAR = REF | PP), also through the round-based loop; pendulum: the script setting and SCP converge mode (k_cl_loop_scp<M, 3>).
    Without a reference that variant of the kernels gets the one-row zero reference."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    P = H.spread_params(m, B, 15.0, seed=9)
    reference = _wavy_reference(m, B, steps + 4, 0.2) if with_reference else None
    if model == "rocket":
        x0, kw = np.tile(m.x_ref + 0.3 * (m.extra["x0"] - m.x_ref), (B, 1)), dict(solve_nominal=True, continuation=2)
    else:
        x0, kw = np.tile(m.extra["x0"], (B, 1)) * (1.0 + 0.2 * np.random.default_rng(3).uniform(-1, 1, (B, 1))), {}
    W = _seeded_W(m, B, steps)
    keys = LOG_KEYS + PP_KEYS + ("qp_stats", "log_model_error")
    ref, ref_fin = _stepwise(_make(m, N, B, rti, rti_steps, reference, tune, P), steps, x0, W, **kw)
    print("success rate", ref["success"].mean(), "disturbance_used > 1:", (ref["disturbance_used"] > 1).mean())
    assert ref["success"].any() and ref["model_error"].any()
    out, fin = _decoupled(_make(m, N, B, rti, rti_steps, reference, tune, P), steps, x0, W, waves=waves, **kw)
    _assert_same(out, fin, ref, ref_fin, "persistent", keys)
    assert out["loop_stats"]["waves"] == (B if waves is None else waves)
    plain, _ = _decoupled(_make(m, N, B, rti, rti_steps, reference, tune), steps, x0, W, waves=waves, **kw)
    assert not np.array_equal(plain["state_trajectory"], out["state_trajectory"])      # the parameters are in use
    assert np.array_equal(plain["state_trajectory"][:, :, 0], out["state_trajectory"][:, :, 0]) and "model_error" not in plain
    if model == "rocket":
        def rounds(o):
            o.cl_persistent = 0
        out, fin = _decoupled(_make(m, N, B, rti, rti_steps, reference, rounds, P), steps, x0, W, **kw)
        _assert_same(out, fin, ref, ref_fin, "rounds", keys)


# ---- 4: shared = equal rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [_stepwise, _decoupled])
def test_shared_vector_and_equal_rows_are_the_same_bits(run):
    from robust_nonlinear_mpc_amd import get_model, plant_param_defaults
    m = get_model("pendulum")
    N, B, steps = 10, 5, 4
    p = plant_param_defaults(m) * np.array([1.2, 0.8, 1.1, 1.0])
    x0, W = _x0(m, B), _seeded_W(m, B, steps)
    ref, ref_fin = run(_make(m, N, B, plant_params=p), steps, x0, W)
    out, fin = run(_make(m, N, B, plant_params=np.tile(p, (B, 1))), steps, x0, W)
    assert ref["success"].any() and ref["model_error"].any()
    _assert_same(out, fin, ref, ref_fin, run.__name__, LOG_KEYS + PP_KEYS + ("qp_stats", "log_model_error"))
    out, fin = run(_make(m, N, B, plant_params={"m1": p[0], "m2": np.full(B, p[1]), "l": p[2]}), steps, x0, W)
    _assert_same(out, fin, ref, ref_fin, run.__name__ + " dict", LOG_KEYS + PP_KEYS + ("qp_stats", "log_model_error"))


# ---- 5: against the CPU oracle loop ---------------------------------------------------------------------------------------------------------
def test_closed_loop_vs_oracle_with_mismatched_plant():
    """Pendulum at the script settings, 6 steps, two instances with different parameters, against the CPU restatement whose plant step is the host's
    ddyn_p while its controller keeps the numpy restatement of the model: the 1e-6 relative of test_tracked_closed_loop_vs_oracle."""
    from robust_nonlinear_mpc_amd import get_model, plant_param_defaults
    m = get_model("pendulum")
    N, steps, B = 10, 6, 2
    P = plant_param_defaults(m)[None, :] * np.array([[1.25, 0.8, 1.15, 1.0], [0.8, 1.3, 0.9, 1.02]])
    x0 = np.tile(m.extra["x0"], (B, 1))
    cl = _make(m, N, B, plant_params=P)
    out = cl.run_on_device(x0, steps)
    cl.close()
    for b in range(B):
        ref = H.run_oracle_closed_loop_plant(m, N, x0[b], steps, m.rti, m.fast_sls_rti_steps, lambda x, u: H.host_ddyn_p(m.model_id, x, u, P[b]))
        assert ref["success"].all() and ref["oracle_qp_converged"].all()
        scale = max(1.0, np.abs(ref["nominal_x"]).max())
        uscale = max(1.0, np.abs(ref["nominal_u"]).max())
        errs = dict(
            state=np.max(np.abs(out["state_trajectory"][b].T - ref["state"])) / scale,
            u0=np.max(np.abs(out["input_trajectory"][b].T - ref["u0"][: steps - 1])) / max(1.0, np.abs(ref["u0"]).max()),
            nominal_x=np.max(np.abs(out["nominal_trajectory_x"][b].transpose(2, 1, 0) - ref["nominal_x"])) / scale,
            nominal_u=np.max(np.abs(out["nominal_trajectory_u"][b].transpose(2, 1, 0) - ref["nominal_u"])) / uscale,
            model_error=np.max(np.abs(out["model_error"][b].T - ref["model_error"])) / scale)
        print(b, errs, "largest model error", np.abs(ref["model_error"]).max())
        assert list(out["success"][b]) == list(ref["success"])
        assert np.abs(ref["model_error"]).max() > 1e-4      # 1e-6 separates the mismatched plant from the model
        for k, e in errs.items():
            assert e < 1e-6, (b, k, e)


# ---- 6: Monte-Carlo driver ----------------------------------------------------------------------------------------------------------------
def test_monte_carlo_cuts_per_seed_plant_params_with_the_seeds():
    """6 seeds in two slices equal the two direct runs of seeds 0-2 and 3-5 with their rows, and one slice; a dict with per-seed entries is cut the same way."""
    from robust_nonlinear_mpc_amd import get_model, run_monte_carlo
    m = get_model("quadrotor")
    N, S, steps = 10, 6, 3
    x0 = m.x_ref + 0.02 * (m.x_ub - m.x_lb)
    x0[6:10] /= np.linalg.norm(x0[6:10])
    P = H.spread_params(m, S, 20.0, seed=2)
    kw = dict(noise=True, gather=False)
    two = run_monte_carlo(m, N, np.arange(S), steps, x0, plant_params=P, slices=2, **kw)
    one = run_monte_carlo(m, N, np.arange(S), steps, x0, plant_params=P, **kw)
    lo = run_monte_carlo(m, N, np.arange(0, 3), steps, x0, plant_params=P[:3], **kw)
    hi = run_monte_carlo(m, N, np.arange(3, 6), steps, x0, plant_params=P[3:], **kw)
    plain = run_monte_carlo(m, N, np.arange(S), steps, x0, **kw)
    assert two["success"].any() and two["model_error"].any() and "model_error" not in plain
    assert two["disturbance_used"].shape == (steps, S) and two["model_error"].shape == (S, m.nx, steps) and np.array_equal(two["plant_params"], P)
    for k in LOG_KEYS + ("model_error",):
        assert np.array_equal(two[k], one[k], equal_nan=True), k
        assert np.array_equal(two[k], np.concatenate([lo[k], hi[k]], axis=0), equal_nan=True), k
    assert np.array_equal(two["disturbance_used"], one["disturbance_used"]) and np.array_equal(two["disturbance_used"], np.concatenate([lo["disturbance_used"], hi["disturbance_used"]], axis=1))
    assert not np.array_equal(two["state_trajectory"], plain["state_trajectory"])
    d = run_monte_carlo(m, N, np.arange(S), steps, x0, plant_params={"m": P[:, 0], "Jx": P[:, 3]}, slices=2, **kw)
    e = run_monte_carlo(m, N, np.arange(S), steps, x0, plant_params={"m": P[:, 0], "Jx": P[:, 3]}, **kw)
    for k in LOG_KEYS + ("model_error",):
        assert np.array_equal(d[k], e[k], equal_nan=True), k
    with pytest.raises(ValueError, match="per-seed"):
        run_monte_carlo(m, N, np.arange(S), steps, x0, plant_params=P[:5], **kw)


# ---- 7: refusals ----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_leave_the_parameters_in_force():
    from robust_nonlinear_mpc_amd import BatchedFastSLS, ClosedLoopMPC, get_model, plant_param_defaults
    L = __import__("robust_nonlinear_mpc_amd")._lib
    m = get_model("quadrotor")
    N, B = 8, 3
    d = plant_param_defaults(m)
    P = H.spread_params(m, B, 20.0, seed=4)
    x0 = _x0(m, B)
    cl = ClosedLoopMPC(m, N, B, plant_params=P)
    lib, h = cl.f.lib, cl.f.h

    def step_now():
        cl.reset(x0)
        cl.step(None, fetch=False)
        return cl.f.get("x_meas", (m.nx,)), cl.f.get("model_err", (m.nx,))
    x_ref, e_ref = step_now()
    assert e_ref.any()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    nan = P.copy(); nan[1, 2] = np.nan
    inf = P.copy(); inf[2, 6] = np.inf
    mass0 = P.copy(); mass0[0, 0] = 0.0
    negJ = P.copy(); negJ[2, 4] = -0.02
    short = np.ascontiguousarray(P[:, :6])
    for args, word in (((ptr(short), 6, 1), "np"), ((ptr(P), 8, 1), "np"), ((ptr(nan), 7, 1), "NaN"), ((ptr(inf), 7, 1), "infinite"), ((ptr(mass0), 7, 1), "m ="),
                       ((ptr(negJ), 7, 1), "Jy"), ((ptr(P), 7, 2), "per_instance"), ((ptr(P), -1, 1), "np"), ((None, 7, 0), "NULL"), ((ptr(P), 0, 0), "clears")):
        assert lib.slsqp_cl_set_plant_params(h, *args, L.HOST) < 0, (args, word)
        assert word in lib.slsqp_last_error().decode(), (word, lib.slsqp_last_error().decode())
        x, e = step_now()
        assert np.array_equal(x, x_ref) and np.array_equal(e, e_ref), word
    # the Python layer: per-instance array of the wrong batch, unknown name, zero mass by name
    for bad in (np.tile(d, (B + 1, 1)), {"weight": 1.0}, d[:-1]):
        with pytest.raises(ValueError):
            cl.set_plant_params(bad)
    with pytest.raises(RuntimeError, match="> 0"):
        cl.set_plant_params({"m": 0.0})
    with pytest.raises(RuntimeError, match="> 0"):
        cl.set_plant_params({"Jz": np.array([0.04, -0.04, 0.04])})
    x, e = step_now()
    assert np.array_equal(x, x_ref) and np.array_equal(e, e_ref) and np.array_equal(cl.f.get("plant_params", (7,)), P)
    cl.set_plant_params({"kM": -0.01})      # the yaw moment coefficient only has to be finite
    assert not np.array_equal(step_now()[0], x_ref)
    cl.close()
    # a handle without a model
    mk = get_model("pendulum")
    src = type("NoPlant", (), dict(nx=mk.nx, nu=mk.nu, nw=mk.nw, ni=mk.ni, ni_f=mk.ni_f, G=mk.G, Gf=mk.Gf, gf=mk.gf, E=mk.E))()
    f = BatchedFastSLS(N, mk.Q, mk.R, src, mk.Qf, batch=2)
    dp = plant_param_defaults(mk)
    assert f.lib.slsqp_cl_set_plant_params(f.h, ptr(dp), 4, 0, L.HOST) < 0 and "slsqp_set_model" in f.lib.slsqp_last_error().decode()
    with pytest.raises(RuntimeError, match="slsqp_set_model"):
        f.set_plant_params(dp)
    f.close()
    assert lib.slsqp_plant_param_count(3) == -1 and lib.slsqp_plant_param_name(1, 7) is None and lib.slsqp_plant_param_name(2, 0) == b"mass"


# ---- 8: debug allocators --------------------------------------------------------------------------------------------------------------------
def test_setter_under_debug_allocators():
    """slsqp_cl_set_plant_params, the queries and the three new slsqp_get names with host buffers of exactly the documented sizes, in a child process
    whose allocators check their block boundaries (as tests/test_gpu_reference.py::test_setter_under_debug_allocators)."""
    env = dict(os.environ, MALLOC_CHECK_="3", PYTHONMALLOC="malloc_debug")
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.join(ROOT, "tests", "abi_memcheck_plant.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "abi_memcheck_plant ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

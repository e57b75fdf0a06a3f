"""The SLS sweep (Riccati recursion, Phi propagation, row norms beta, back-offs, tightened bounds, cost_tube) on every route a solve can take
through it, each held against tests/sweep_ref.py -- a plain np.longdouble restatement, itself pinned on the CPU by tests/test_sweep_ref_cpu.py --
on the eta the device itself used: after a solve the test fetches eta, eta_f, A, Bm, c, g, runs the restatement on exactly those and compares K,
beta, beta_f, backoff, backoff_f, backoff_x, backoff_u, ubg and cost_tube.  A kernel against a high-precision reference of the same operation on the
same inputs; the QP solver's accuracy does not enter.  Tolerance: the project's sweep tolerance, 1e-9 max-norm relative (1e-9 max(1, want) for
cost_tube); K and beta above the diagonal (j > k) are exactly 0.

Routes:  a  rti_steps = 1, separate launches (k_after_qp -> k_sweep_ric1 + k_sweep_prop -> k_tighten), 11 instances
         b  rti_steps = 1, the fused chain (k_rti_chain), bit for bit route a
         c  rti_steps = 2 with conv_tol = -1: the second iteration always sweeps, through k_sweep with a per-column eta, 11 instances
         d  the per-column kernel (slsqp_sweep on a second handle) on route a's eta against route a's shared kernels
         e  converge mode: eta of the last step from the dual and the beta of the same fetch, to 1e-14
         f  a second call on unchanged data: not swept (quirk q5), beta repaired to eps
         closed loops (k_cl_loop / k_cl_loop_scp against the step-by-step loop) with a stage-varying E
Inputs: tests/sweep_cases.py (smallest shapes that reach every branch; the model's E, a dense stage-varying E, a dense nw < nx E; constraints active).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import sweep_ref as SR
from problems import make_gpu_solver, push_instances, stack
from sweep_cases import ALL_CASES, B_MAX, case_id, dense_E, make_case
from test_gpu_cl_scp import _assert_same, _persistent, _seeded_W, _stepwise

pytestmark = pytest.mark.gpu

TOL = 1e-9
EPS = 1e-10
IDS = [case_id(*c) for c in ALL_CASES]
relerr = SR.relerr


def fetch(f):
    """Everything the checks read, from the handle as it stands."""
    m, N = f.m, f.N
    nx, nu, ni, nif = m.nx, m.nu, m.ni, m.ni_f
    shapes = dict(eta=(N, N, ni), eta_f=(N + 1, nif), A=(N, nx, nx), Bm=(N, nx, nu), c=(N, nx), g=(N, ni), K=(N, N + 1, nu, nx), beta=(N, N, ni),
                  beta_f=(N + 1, nif), backoff=(N, ni), backoff_f=(nif,), backoff_x=(N + 1, nx), backoff_u=(N, nu), ubg=(f.mb,), cost_tube=(),
                  primal_vec=(f.n,), dual_vec=(f.mb,))
    out = {k: f.get(k, s) for k, s in shapes.items()}
    for k in ("iteration_number", "success", "status"):
        out[k] = f.get(k, (), np.int32)
    return out


def solve(insts, rti_steps, fuse_rti, conv_tol=None, calls=1):
    f = make_gpu_solver(insts)
    f.set_rti_steps(rti_steps)
    f.opts.fuse_rti = fuse_rti
    if conv_tol is not None:
        f.opts.conv_tol = conv_tol
    for _ in range(calls):
        push_instances(f, insts)
        f.solve(stack(insts, "x0_arg"), fetch=False)
    r = fetch(f)
    f.close()
    return r


def check_sweep(r, m, E, which=None, label=""):
    """The consistency statement: the device's sweep results are the sweep of the eta, A, B, c, g the device holds.  All instances unless `which`."""
    B, N = r["eta"].shape[0], r["eta"].shape[1]
    worst = {}
    for b in (range(B) if which is None else which):
        ref = SR.sweep(r["A"][b], r["Bm"][b], E, m.G, m.Gf, r["eta"][b], r["eta_f"][b], m.Q_reg, m.R_reg, m.Q_reg_f, EPS, c=r["c"][b], g=r["g"][b],
                       gf_raw=m.gf)
        for k in ("K", "beta", "beta_f", "backoff", "backoff_f", "backoff_x", "backoff_u", "ubg"):
            e = relerr(r[k][b], ref[k])
            worst[k] = max(worst.get(k, 0.0), e)
            assert e < TOL, (label, b, k, e)
        want = float(ref["cost_tube"])
        e = abs(r["cost_tube"][b] - want) / max(1.0, want)
        worst["cost_tube"] = max(worst.get("cost_tube", 0.0), e)
        assert e < TOL, (label, b, "cost_tube", r["cost_tube"][b], want)
        for k in range(N):
            assert not r["K"][b, k, k + 1:].any() and not r["beta"][b, k, k + 1:].any(), (label, b, k, "above the diagonal")
    print(label, "largest relative errors against the longdouble sweep:", {k: f"{v:.1e}" for k, v in worst.items()})


def check_broadcast(r, K_too=True):
    """What slsqp_get hands out after a first fast-SLS iteration: column 0 of eta in every column j <= k (zeros above), row 0 of eta_f in every row,
    the compact K_k in every column j <= k -- bit for bit."""
    N = r["eta"].shape[1]
    for k in range(N):
        for j in range(N):
            assert np.array_equal(r["eta"][:, k, j], r["eta"][:, k, 0] if j <= k else np.zeros_like(r["eta"][:, k, 0])), ("eta", k, j)
        for j in range(N + 1):
            if K_too:
                assert np.array_equal(r["K"][:, k, j], r["K"][:, k, 0] if j <= k else np.zeros_like(r["K"][:, k, 0])), ("K", k, j)
    for j in range(N + 1):
        assert np.array_equal(r["eta_f"][:, j], r["eta_f"][:, 0]), ("eta_f", j)


@functools.lru_cache(maxsize=None)
def route_a(model, N, variant):
    """rti_steps = 1 through the separate launches, 11 instances: computed once per input set, shared by the tests of routes a, b and d."""
    insts = make_case(model, N, variant, B_MAX)
    r = solve(insts, 1, 0)
    for v in r.values():
        v.setflags(write=False)
    return insts, r


@pytest.mark.parametrize("model,N,variant", ALL_CASES, ids=IDS)
def test_route_a_separate_launches(model, N, variant):
    insts, r = route_a(model, N, variant)
    assert r["success"].all() and (r["iteration_number"] == 1).all() and np.isin(r["status"], (0, 4)).all(), (r["success"], r["iteration_number"], r["status"])
    assert r["eta"][:3].any()                   # constraints are active: the Riccati recursion sees a state / input weight from eta
    check_broadcast(r)
    check_sweep(r, insts[0].m, insts[0].E, label=f"route a {case_id(model, N, variant)}")


@pytest.mark.parametrize("model,N,variant", ALL_CASES, ids=IDS)
def test_route_b_fused_chain_is_bitwise_route_a(model, N, variant):
    insts, ra = route_a(model, N, variant)
    r = solve(insts[:3], 1, 2)
    assert r["success"].all() and (r["iteration_number"] == 1).all()
    check_broadcast(r)
    check_sweep(r, insts[0].m, insts[0].E, label=f"route b {case_id(model, N, variant)}")
    for k in r:
        assert np.array_equal(r[k], ra[k][:3]), k


@pytest.mark.parametrize("model,N,variant", ALL_CASES, ids=IDS)
def test_route_c_second_iteration_through_the_per_column_kernel(model, N, variant):
    insts = make_case(model, N, variant, B_MAX)
    r = solve(insts, 2, 0, conv_tol=-1.0)
    assert r["success"].all() and (r["iteration_number"] == 2).all(), (r["success"], r["iteration_number"])
    check_sweep(r, insts[0].m, insts[0].E, label=f"route c {case_id(model, N, variant)}")
    if N > 1:       # (N = 1: one column of eta) a stale broadcast of column 0 cannot pass: beta differs between the columns, so does eta
        assert (r["eta"][:, N - 1, 0] != r["eta"][:, N - 1, N - 1]).any()
    assert (r["eta_f"][:, 0] != r["eta_f"][:, N]).any() or not r["eta_f"].any()


@pytest.mark.parametrize("model,N,variant", ALL_CASES, ids=IDS)
def test_route_d_shared_kernels_against_the_per_column_kernel(model, N, variant):
    """Route a's eta pushed into slsqp_sweep of a second handle with the same A, B, E and regularisers: k_sweep, one wave per column with its own
    Riccati recursion, against k_sweep_ric1 + k_sweep_prop.  Both are within 1e-9 of the longdouble sweep; the largest relative difference between
    the two kernels measured on an MI355X is 0 on every input set (vector-ALU products of the pendulum and the paired matrix-core products of the
    two larger plants alike), so "the same arithmetic in the same order"  is asserted bit for bit."""
    insts, ra = route_a(model, N, variant)
    m, E = insts[0].m, insts[0].E
    f = make_gpu_solver(insts[:3])
    push_instances(f, insts[:3])
    out = f.sweep(ra["eta"][:3], ra["eta_f"][:3])
    f.close()
    diff = 0.0
    for b in range(3):
        ref = SR.sweep(ra["A"][b], ra["Bm"][b], E, m.G, m.Gf, ra["eta"][b], ra["eta_f"][b], m.Q_reg, m.R_reg, m.Q_reg_f, EPS)
        for k in ("K", "beta", "beta_f", "backoff", "backoff_f"):
            assert relerr(out[k][b], ref[k]) < TOL and relerr(ra[k][b], ref[k]) < TOL, (b, k)
            diff = max(diff, relerr(out[k][b], ra[k][b]))
        assert abs(out["cost_tube_value"][b] - float(ref["cost_tube"])) < TOL * max(1.0, float(ref["cost_tube"]))
    print(f"route d {case_id(model, N, variant)}: largest relative difference shared vs per-column kernel {diff:.3e}")
    for k in ("K", "beta", "beta_f", "backoff", "backoff_f"):
        assert np.array_equal(out[k], ra[k][:3]), k
    assert np.array_equal(out["cost_tube_value"], ra["cost_tube"][:3])


@pytest.mark.parametrize("model,N", [("quadrotor", 2), ("rocket", 3)])
def test_general_G_sweep_at_the_matrix_core_dimension_pairs(model, N):
    """k_sweep_gen at (13, 4) and (17, 4): the only general-G fixture (tests/test_gpu_parity.py) is the pendulum's, (4, 1).  A general G
    (2 nz + 3 rows) and Gf (2 nx + 1 rows), N(0, 1) / sqrt(nz) entries below the model's [I; -I] rows (so that C_uu + R_reg stays well conditioned),
    eta and eta_f uniform at the scale of route a's eta for the same input set, pushed into slsqp_sweep and held against the longdouble sweep on
    the same arrays, every instance."""
    from types import SimpleNamespace
    from robust_nonlinear_mpc_amd import BatchedFastSLS
    B = 3
    insts = make_case(model, N, "dense", B)
    base, E = insts[0].m, insts[0].E
    nx, nu, nz = base.nx, base.nu, base.nz
    ni, nif = 2 * nz + 3, 2 * nx + 1
    rng = np.random.default_rng(1900 + nx)
    G, Gf = rng.normal(size=(ni, nz)) / np.sqrt(nz), rng.normal(size=(nif, nx)) / np.sqrt(nz)
    G[:2 * nz], Gf[:2 * nx] = base.G, base.Gf
    scale = float(np.abs(route_a(model, N, "dense")[1]["eta"]).max()) or 1.0
    eta, eta_f = scale * rng.uniform(size=(B, N, N, ni)), scale * rng.uniform(size=(B, N + 1, nif))
    m = SimpleNamespace(nx=nx, nu=nu, nw=base.nw, ni=ni, ni_f=nif, G=G, Gf=Gf, gf=np.zeros(nif), E=base.E, Q=base.Q, R=base.R, Qf=base.Qf)
    f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, base.Q_reg, base.R_reg, base.Q_reg_f, batch=B)
    A, Bm = stack(insts, "A"), stack(insts, "B")
    f.update_dynamics_list(A, Bm, E, np.zeros((B, N, ni)), np.zeros((B, nif)), np.zeros((B, N, nx)))
    out = f.sweep(eta, eta_f)
    f.close()
    worst = {}
    for b in range(B):
        ref = SR.sweep(A[b], Bm[b], E, G, Gf, eta[b], eta_f[b], base.Q_reg, base.R_reg, base.Q_reg_f, EPS)
        want = float(ref["cost_tube"])
        errs = {k: relerr(out[k][b], ref[k]) for k in ("K", "beta", "beta_f", "backoff", "backoff_f")}
        errs["cost_tube"] = abs(out["cost_tube_value"][b] - want) / max(1.0, want)
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
        print(f"general G {model} N{N} instance {b}:", {k: f"{e:.1e}" for k, e in errs.items()})
        for k, e in errs.items():
            assert e < TOL, (b, k, e)
    print(f"general G {model} N{N} (eta scale {scale:.3g}) largest relative errors against the longdouble sweep:", {k: f"{v:.1e}" for k, v in worst.items()})


@pytest.mark.parametrize("model,N", [("pendulum", 5), ("quadrotor", 5)])
@pytest.mark.parametrize("variant", ["model", "dense", "nw"])
def test_route_e_converge_mode_eta_is_exact(model, N, variant):
    """rti_steps = 0: an instance that reports success left at a step whose QP moved less than conv_tol; that step computed eta from its dual and the
    beta of the last sweep, and nothing was written afterwards.  So eta[k,j] = mu_k / (2 sqrt(max(beta[k,j], eps))) from the same fetch, to 1e-14
    relative: a handful of correctly rounded fp64 operations.  (No sweep check here: the last sweep ran on the previous step's eta, which the handle
    no longer holds.)"""
    insts = make_case(model, N, variant, 3)
    m = insts[0].m
    r = solve(insts, 0, 0)
    ok = np.flatnonzero(r["success"] & (r["iteration_number"] >= 1))
    print("converge mode: success", r["success"], "iterations", r["iteration_number"])
    assert len(ok) >= 1
    for b in ok:
        dv = r["dual_vec"][b]
        mu = dv[:-m.ni_f].reshape(N, m.nx + m.ni)[:, m.nx:]          # (N, ni)
        mu_f = dv[-m.ni_f:]
        for k in range(N):
            for j in range(N):
                want = mu[k] / (2.0 * np.sqrt(np.maximum(r["beta"][b, k, j], EPS))) if j <= k else np.zeros(m.ni)
                assert np.allclose(r["eta"][b, k, j], want, rtol=1e-14, atol=0.0), (b, k, j)
        for j in range(N + 1):
            assert np.allclose(r["eta_f"][b, j], mu_f / (2.0 * np.sqrt(np.maximum(r["beta_f"][b, j], EPS))), rtol=1e-14, atol=0.0), (b, j)
        assert r["eta"][b].any()


@pytest.mark.parametrize("fuse_rti", [0, 2])
@pytest.mark.parametrize("model,N,variant", [("pendulum", 5, "dense"), ("rocket", 3, "nw")])
def test_route_f_the_instance_that_is_not_swept(model, N, variant, fuse_rti):
    """A second rti_steps = 1 call on unchanged data: the first QP repeats the previous call's, the convergence test passes, the sweep is skipped
    (quirk q5) and k_after_qp puts initialize_backoff's eps back into the beta the first call's sweep wrote."""
    insts = make_case(model, N, variant, 3)
    m = insts[0].m
    r = solve(insts, 1, fuse_rti, calls=2)
    assert r["success"].all() and (r["iteration_number"] == 1).all()          # not incremented by the second call
    assert np.array_equal(r["beta"], np.full_like(r["beta"], EPS)) and np.array_equal(r["beta_f"], np.full_like(r["beta_f"], EPS))
    assert np.array_equal(r["backoff"], np.full_like(r["backoff"], N * np.sqrt(EPS)))
    assert np.array_equal(r["backoff_f"], np.full_like(r["backoff_f"], (N + 1) * np.sqrt(EPS)))
    assert not r["backoff_x"].any() and not r["backoff_u"].any()
    assert r["eta"].any()
    check_broadcast(r, K_too=False)
    dv = r["dual_vec"]
    mu = dv[:, :-m.ni_f].reshape(3, N, m.nx + m.ni)[:, :, m.nx:]
    assert np.allclose(r["eta"][:, :, 0], mu / (2.0 * np.sqrt(EPS)), rtol=1e-14, atol=0.0)


@pytest.mark.parametrize("conv_tol", [None, -1.0], ids=["conv_tol_default", "always_sweep"])
@pytest.mark.parametrize("model,N,B,steps", [("pendulum", 10, 24, 4), ("rocket", 6, 16, 3)])
def test_closed_loops_with_a_stage_varying_E(model, N, B, steps, conv_tol):
    """The persistent closed-loop kernels (k_cl_loop for the rocket's one iteration / one step, k_cl_loop_scp for the pendulum's 3 x 2) against the
    step-by-step loop, bit for bit, at the scripts' rti / fast_sls_rti_steps with E_0 = the model's E (all the plant step reads) and dense, different
    later stages, set through slsqp_set_E on both sides.  Then the consistency statement on the step-by-step side's final state, for the instances
    whose last fast-SLS iteration swept: every one of the step's rti x rti_steps iterations did (iteration_number counts them).  With the default
    conv_tol later SCP iterations move less than 1e-3 and skip their sweeps (quirk q5); conv_tol = -1 makes every iteration sweep."""
    from robust_nonlinear_mpc_amd import get_model
    L = __import__("robust_nonlinear_mpc_amd")._lib
    m = get_model(model)
    E = dense_E(m, N)
    assert np.array_equal(E[0], m.E)
    rng = np.random.default_rng(11)
    x0 = np.stack([m.x_ref + (1.0 if model == "pendulum" else 0.3) * 0.05 * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, m.nx) for _ in range(B)])
    W = _seeded_W(m, B, steps)
    seen = {}

    def tune(o):
        if conv_tol is not None:
            o.conv_tol = conv_tol

    def setup(cl):
        L.check(cl.f.lib.slsqp_set_E(cl.f.h, np.ascontiguousarray(E).ctypes.data_as(C.c_void_p), L.HOST))

    def inspect(cl):
        seen.update(fetch(cl.f))
        seen["scp_success"] = cl.f.get("scp_success", (), np.int32)

    ref, ref_fin = _stepwise(m, N, B, steps, x0, W, None, None, tune, setup=setup, inspect=inspect)
    out, fin = _persistent(m, N, B, steps, x0, W, None, None, tune, setup=setup)
    _assert_same(out, fin, ref, ref_fin, B, steps)
    assert ref["success"].mean() > 0.5
    swept = np.flatnonzero((seen["scp_success"] != 0) & (seen["iteration_number"] == m.rti * m.fast_sls_rti_steps))
    print("last step: scp_success", seen["scp_success"], "sweeps", seen["iteration_number"], "checked", swept)
    if conv_tol is not None:
        assert len(swept) == np.count_nonzero(seen["scp_success"]) and len(swept) >= 1
    check_sweep(seen, m, E, which=swept, label=f"closed loop {model} conv_tol {conv_tol}")

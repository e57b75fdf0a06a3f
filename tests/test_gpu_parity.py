"""GPU parity tests: the HIP path (through the C-ABI) against the CPU oracle on the same seeded inputs.

Tolerances (north_star: trajectories to 1e-6 rel):
  sweep (K, beta, back-offs) vs the golden vectors of the reference's own kernels: 1e-9 rel
  QP primal vs oracle (OSQP restatement driven to eps 1e-9 + polish): 1e-6 rel; KKT certificate <= 1e-8
  full fast-SLS step (2 QPs + sweep): primal 1e-6 rel, back-offs 1e-6 rel
"""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN
from problems import (make_instance, make_gpu_solver, oracle_dims, push_instances, qp1_bounds, run_gpu_fastsls,
                      run_oracle_fastsls, stack)

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b)))


SWEEP_CASES = ["sweep_pendulum_N10_s0.npz", "sweep_pendulum_N3_s2.npz", "sweep_quadrotor_N20_s0.npz", "sweep_rocket_N20_s0.npz",
               "sweep_rocket_N5_s1.npz", "sweep_pendulum_N10_s1_genG.npz", "sweep_pendulum_N6_s4_nw2.npz", "sweep_quadrotor_N8_s3_nw5.npz"]


@pytest.mark.parametrize("case", SWEEP_CASES)
def test_sweep_vs_reference_golden(case):
    from robust_nonlinear_mpc_amd import BatchedFastSLS, get_model
    g = dict(np.load(os.path.join(GOLDEN, case)))
    name = case.split("_")[1]
    m = get_model(name)
    N = int(g["N"])
    B = 3
    if "genG" in case:
        # a model with a general constraint matrix (7 x 5 and 5 x 4 random rows; the reference's kernels take any G, fast_SLS_jit.py:76-79,
        # 138-170): the sweep-level boundary accepts it (k_sweep_gen), the QP-level entry points refuse it loudly
        from types import SimpleNamespace
        base = m
        m = SimpleNamespace(nx=base.nx, nu=base.nu, nw=base.nw, ni=int(g["ni"]), ni_f=int(g["ni_f"]), G=g["G"], Gf=g["Gf"], gf=np.zeros(int(g["ni_f"])),
                            E=base.E, Q=base.Q, R=base.R, Qf=base.Qf)
    if "_nw" in case:
        # fewer disturbance channels than states (nw < nx; dyn/LTV.py:17-32 takes any nw, fast_SLS_jit.py:104-108): dense nx x nw blocks E_j that
        # differ per stage, golden vectors from the reference's own kernels
        from types import SimpleNamespace
        base = m
        m = SimpleNamespace(nx=base.nx, nu=base.nu, nw=int(g["nw"]), ni=base.ni, ni_f=base.ni_f, G=base.G, Gf=base.Gf, gf=base.gf, E=g["E"][0], Q=base.Q, R=base.R,
                            Qf=base.Qf)
        assert m.nw < m.nx and g["E"].shape == (N + 1, m.nx, m.nw)
    f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, g["Q_reg"], g["R_reg"], g["Q_reg_f"], batch=B)
    rng = np.random.default_rng(5)
    # instance 0 = the golden case; the others are perturbed copies (must not disturb instance 0)
    A = np.stack([g["A"]] + [g["A"] + 1e-2 * rng.normal(size=g["A"].shape) for _ in range(B - 1)])
    Bm = np.stack([g["B"]] * B)
    zeros = lambda *s: np.zeros(s)
    f.update_dynamics_list(A, Bm, g["E"], zeros(B, N, m.ni), zeros(B, m.ni_f), zeros(B, N, m.nx))
    out = f.sweep(np.stack([g["eta"]] * B), np.stack([g["eta_f"]] * B))
    if "genG" in case:
        with pytest.raises(RuntimeError, match="general G"):
            f.solve(np.zeros((B, m.nx)))
    f.close()
    assert relerr(out["K"][0], g["K"]) < 1e-9
    assert relerr(out["beta"][0], g["beta"]) < 1e-9
    assert relerr(out["beta_f"][0], g["beta_f"]) < 1e-9
    assert relerr(out["backoff"][0], g["backoff"]) < 1e-9
    assert relerr(out["backoff_f"][0], g["backoff_f"]) < 1e-9
    assert relerr(out["K"][1], g["K"]) > 1e-6  # perturbed instance really differs
    # cost_tube = || blkdiag(Q_reg x N, Q_reg_f, R_reg x N) [Phi_x; Phi_u] ||_F (util/SLS.py:38-46, fast_SLS_jit.py:540-544), from the
    # reference's own Phi where the fixture holds it, else from its block Frobenius norms (the regularisers are multiples of I)
    want = None
    if "Phi_x" in g:
        qd, rd, qfd = np.diag(g["Q_reg"]), np.diag(g["R_reg"]), np.diag(g["Q_reg_f"])
        Px, Pu = g["Phi_x"], g["Phi_u"]
        want = np.sqrt(sum((((qd if k < N else qfd)[:, None] * Px[k, j]) ** 2).sum() for k in range(N + 1) for j in range(N + 1))
                       + sum(((rd[:, None] * Pu[k, j]) ** 2).sum() for k in range(N) for j in range(N + 1)))
    else:
        q, r, qf = g["Q_reg"][0, 0], g["R_reg"][0, 0], g["Q_reg_f"][0, 0]
        if np.allclose(g["Q_reg"], q * np.eye(m.nx)) and np.allclose(g["R_reg"], r * np.eye(m.nu)) and np.allclose(g["Q_reg_f"], qf * np.eye(m.nx)):
            want = np.sqrt(((q * g["Phix_fro"][:N]) ** 2).sum() + ((qf * g["Phix_fro"][N]) ** 2).sum() + ((r * g["Phiu_fro"]) ** 2).sum())
    if want is not None:
        assert abs(out["cost_tube_value"][0] - want) < 1e-9 * max(1.0, want)


def test_extra_dims_build():
    """The (nx, nu) pairs the kernels exist for are a build-time list (csrc/slsqp_api.hip SLSQP_DIM_LIST; -DSLSQP_EXTRA_DIMS adds pairs):
    __graft_entry__.build() also builds libslsqp_hip_dims62.so with (6,2) added, and a fast-SLS step of a random (6,2) plant solved through
    it matches the oracle (child process: the library is chosen at import time)."""
    import subprocess
    import sys
    from conftest import ROOT
    so = os.path.join(ROOT, "robust-nonlinear-mpc_amd", "csrc", "libslsqp_hip_dims62.so")
    assert os.path.exists(so), "run __graft_entry__.build()"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dims_extra_check.py")], env=dict(os.environ, SLSQP_SO=so), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "extra dims ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    from robust_nonlinear_mpc_amd import BatchedFastSLS
    from types import SimpleNamespace
    nx, nu = 6, 2
    m = SimpleNamespace(nx=nx, nu=nu, nw=nx, ni=16, ni_f=12, G=np.vstack([np.eye(8), -np.eye(8)]), Gf=np.vstack([np.eye(6), -np.eye(6)]), gf=np.ones(12), E=np.eye(6))
    with pytest.raises(RuntimeError, match="unsupported"):      # the default library does not carry (6,2) and says which pairs it has
        BatchedFastSLS(8, np.eye(nx), np.eye(nu), m, np.eye(nx), batch=2)


@pytest.mark.parametrize("model,amps", [("pendulum", (0.2, 1.0)), ("quadrotor", (0.2, 1.0, 2.0)), ("rocket", (0.2, 1.0))])
def test_qp_vs_oracle(model, amps):
    from oracle import oracle as O
    insts = [make_instance(model, s, a) for a in amps for s in range(3)]
    m = insts[0].m
    f = make_gpu_solver(insts)
    push_instances(f, insts)
    lu = [qp1_bounds(i) for i in insts]
    f.qp_update_data_vec(stack(insts, "q"), np.stack([x[0] for x in lu]), np.stack([x[1] for x in lu]))
    x, y, st, it, _ = f.qp_solve()
    f.close()
    for b, inst in enumerate(insts):
        d = oracle_dims(inst)
        l, u = lu[b]
        xo, yo, info = O.qp_solve(d, inst.A, inst.B, m.G, m.Gf, m.Q, m.R, m.Qf, inst.q, l, u, O.tight_settings())
        assert st[b] == 0, f"instance {b}: status {st[b]} after {it[b]} its"
        k = O.qp_kkt(d, inst.A, inst.B, m.G, m.Gf, m.Q, m.R, m.Qf, inst.q, l, u, x[b], y[b])
        scale = max(1.0, np.abs(inst.q).max())
        assert k["stationarity"] < 1e-8 * scale and k["primal"] < 1e-8 and k["dual_sign"] < 1e-8 and k["complementarity"] < 1e-7 * scale, k
        if info.status == 1 and info.polish_status == 1:
            assert relerr(x[b], xo) < 1e-6
            act = np.abs(yo[: -m.nx]) > 1e-6
            assert np.allclose(y[b][: -m.nx][act], yo[: -m.nx][act], rtol=1e-5, atol=1e-6 * scale)


@pytest.mark.parametrize("model,N", [("pendulum", 1), ("pendulum", 32), ("pendulum", 64), ("quadrotor", 7), ("rocket", 15), ("rocket", 40)])
def test_other_horizons_vs_oracle(model, N):
    """Horizon edge cases: N = 1 (a single stage), N = 32 and the ABI's maximum N = 64, an odd horizon, a rocket horizon twice the headline's (the
    script takes any --N, main_rocket...:458-461), and N = 15, the rocket script's own default
    (expe/main_rocket_robust_closed_loop.py:63).  One RTI fast-SLS step (2 QPs + sweep) against the oracle."""
    insts = [make_instance(model, s, 0.1 if N > 32 else 0.5, N=N) for s in range(2)]      # (the open-loop unstable pendulum over 64 stages: a smaller x0)
    out = run_gpu_fastsls(insts, rti_steps=1)
    for b, inst in enumerate(insts):
        ref = run_oracle_fastsls(inst, rti_steps=1)
        assert bool(out["success"][b]) == bool(ref["success"]) and ref["success"]
        assert out["primal_vec"].shape[1] == inst.m.nz * N + inst.m.nx
        assert relerr(out["primal_vec"][b], ref["primal_vec"]) < 1e-6
        assert relerr(out["backoff"][b], ref["backoff"]) < 1e-6
        assert relerr(out["beta_f"][b], ref["beta_f"]) < 1e-6


def test_qp_csc_boundary_matches_dense_boundary():
    """update_data_mat(P_x, A_x) in the reference's CSC order (qp_jit.py:671-698) == update_dynamics with dense blocks."""
    import scipy.sparse as sp
    inst = make_instance("pendulum", 0, 1.0)
    m, N = inst.m, inst.N
    nx, nu, nz, ni = m.nx, m.nu, m.nz, m.ni
    rows = []
    n = m.n_var(N)
    M = np.zeros((m.m_con(N), n))
    r = 0
    for k in range(N):
        M[r:r + nx, k * nz:k * nz + nx] = inst.A[k]; M[r:r + nx, k * nz + nx:(k + 1) * nz] = inst.B[k]
        M[r:r + nx, (k + 1) * nz:(k + 1) * nz + nx] = -np.eye(nx); r += nx
        M[r:r + ni, k * nz:(k + 1) * nz] = m.G; r += ni
    M[r:r + m.ni_f, N * nz:] = m.Gf; r += m.ni_f
    M[r:r + nx, :nx] = np.eye(nx)
    pattern = (M != 0)
    for k in range(N):  # frozen dense pattern of A_k,B_k (qp_jit.py:90-99)
        pattern[k * (nx + ni):k * (nx + ni) + nx, k * nz:(k + 1) * nz] = True
    coo = sp.coo_matrix(pattern)
    csc = sp.csc_matrix((M[coo.row, coo.col], (coo.row, coo.col)), shape=M.shape)
    csc.sort_indices()
    f = make_gpu_solver([inst])
    nn, mm, nP, nA = f.qp_nnz()
    assert (nn, mm, nA) == (54, 152, 352) and csc.nnz == nA  # n, m, nnz(A) of pendulum N=10
    l, u = qp1_bounds(inst)
    Hd = 2 * np.concatenate([np.concatenate([np.diag(m.Q), np.diag(m.R)])] * N + [np.diag(m.Qf)])
    f.qp_update_data_mat(Hd[None], csc.data[None])
    f.qp_update_data_vec(inst.q[None], l[None], u[None])
    x1, y1, st1, _, _ = f.qp_solve()
    push_instances(f, [inst])
    f.qp_update_data_vec(inst.q[None], l[None], u[None])
    x2, y2, st2, _, _ = f.qp_solve()
    f.close()
    assert st1[0] == 0 and st2[0] == 0
    assert np.allclose(x1, x2, rtol=0, atol=1e-12) and np.allclose(y1, y2, rtol=0, atol=1e-10)


@pytest.mark.parametrize("model,rti", [("pendulum", 1), ("pendulum", 2), ("quadrotor", 2), ("rocket", 1)])
def test_fastsls_step_vs_oracle(model, rti):
    insts = [make_instance(model, s, a) for a in (0.3, 1.0) for s in range(2)]
    out = run_gpu_fastsls(insts, rti_steps=rti)
    for b, inst in enumerate(insts):
        ref = run_oracle_fastsls(inst, rti_steps=rti)
        assert bool(out["success"][b]) == bool(ref["success"])
        if not ref["success"]:
            continue
        assert out["iteration_number"][b] == ref["iteration_number"]
        assert relerr(out["primal_vec"][b], ref["primal_vec"]) < 1e-6
        assert relerr(out["backoff"][b], ref["backoff"]) < 1e-6
        assert relerr(out["backoff_f"][b], ref["backoff_f"]) < 1e-6
        assert relerr(out["backoff_x"][b], ref["backoff_x"]) < 1e-6
        assert relerr(out["beta"][b], ref["beta"]) < 1e-6
        assert relerr(out["beta_f"][b], ref["beta_f"]) < 1e-6
        # eta, eta_f and K: full (N,N,ni) / (N+1,ni_f) / (N,N+1,nu,nx) arrays as the reference returns them -- after a single fast-SLS iteration the
        # device holds only column 0 of eta and the compact K_k of the shared Riccati recursion, and slsqp_get broadcasts them on demand
        assert relerr(out["eta"][b], ref["eta"]) < 1e-5 and relerr(out["eta_f"][b], ref["eta_f"]) < 1e-5
        assert relerr(out["K"][b], ref["K"]) < 1e-6
        assert np.allclose(out["primal_x"][b], ref["primal_x"], rtol=1e-6, atol=1e-7)
        assert np.allclose(out["primal_u"][b], ref["primal_u"], rtol=1e-6, atol=1e-7)
        assert abs(out["cost_nominal"][b] - ref["cost_nominal"]) < 1e-6 * max(1.0, abs(ref["cost_nominal"]))


def test_convergence_state_leaks_across_calls_quirk_q5():
    """Second RTI call with (almost) the same primal: _step returns True, Riccati + tightening are skipped and the
    back-offs stay at their initial N*1e-5 values (fast_SLS_jit.py:318-320, 444-454)."""
    insts = [make_instance("pendulum", s, 0.5) for s in range(2)]
    f = make_gpu_solver(insts)
    out1 = run_gpu_fastsls(insts, rti_steps=1, solver=f)
    out2 = run_gpu_fastsls(insts, rti_steps=1, solver=f)
    f.close()
    N = insts[0].N
    assert np.all(out1["iteration_number"] == 1)
    assert np.all(out2["iteration_number"] == 1)          # not incremented: tightening skipped
    assert np.allclose(out2["backoff"], N * 1e-5)
    assert np.allclose(out2["backoff_x"], 0.0)
    assert np.all(out2["success"])


@pytest.mark.parametrize("model", ["pendulum", "quadrotor", "rocket"])
def test_linearize_vs_reference_dynamics(model):
    """slsqp_linearize (forward-mode AD through RK4 on the GPU) against the golden fixtures: c_k from the reference's own ddyn
    values (1e-12), A_k/B_k against central differences of the reference's ddyn (1e-6), g_k, g_N and q by their formulas
    (SCP_SLS_jit.py:348-366)."""
    from robust_nonlinear_mpc_amd import BatchedFastSLS, get_model
    g = dict(np.load(os.path.join(GOLDEN, f"dyn_{model}.npz")))
    m = get_model(model)
    P = g["X"].shape[0]
    N = P - 1 if P - 1 <= 32 else 32
    B = 2
    rng = np.random.default_rng(3)
    X = np.stack([g["X"][: N + 1], g["X"][: N + 1] + 0.01 * rng.normal(size=(N + 1, m.nx))])
    U = np.stack([g["U"][:N], g["U"][:N] + 0.01 * rng.normal(size=(N, m.nu))])
    f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=B)
    f.linearize(X, U)
    A, Bm, c = f.get("A", (N, m.nx, m.nx)), f.get("Bm", (N, m.nx, m.nu)), f.get("c", (N, m.nx))
    gk, gN, q = f.get("g", (N, m.ni)), f.get("gN", (m.ni_f,)), f.get("q", (f.n,))
    ubg = f.get("ubg", (f.mb,))
    f.close()
    assert np.allclose(A[0], g["A_fd"][:N], rtol=1e-6, atol=1e-7)
    assert np.allclose(Bm[0], g["B_fd"][:N], rtol=1e-6, atol=1e-7)
    assert np.allclose(c[0], g["ddyn"][:N] - g["X"][1: N + 1], rtol=0, atol=1e-12)
    Z = np.concatenate([X[:, :N], U], axis=2)
    assert np.allclose(gk, m.g[None, None] - Z @ m.G.T, atol=1e-13)
    assert np.allclose(gN, m.gf[None] - X[:, N] @ m.Gf.T, atol=1e-13)
    Hd = np.concatenate([np.concatenate([np.diag(m.Q), np.diag(m.R)])] * N + [np.diag(m.Qf)])
    ynom = np.concatenate([Z.reshape(B, -1), X[:, N]], axis=1)
    assert np.allclose(q, 2 * Hd[None] * ynom, atol=1e-12)
    SR = m.nx + m.ni
    assert np.allclose(ubg[:, :m.nx], -c[:, 0] + 1e-10, atol=1e-15) and np.allclose(ubg[:, m.nx:SR], gk[:, 0] + 1e-10, atol=1e-14)
    assert not np.allclose(A[1], A[0])


@pytest.mark.parametrize("model,N,steps,amp", [("pendulum", 10, 4, 1.0), ("rocket", 20, 2, 0.3), ("quadrotor", 20, 3, 1.0)])
def test_closed_loop_vs_oracle(model, N, steps, amp):
    """Whole closed-loop MPC steps on the device (linearise -> fast-SLS -> nominal update -> warm-start shift -> plant + noise)
    against the CPU restatement of SCP_SLS.solve / reset_warm_start built on the oracle (its plant and Jacobians: oracle/dyn_oracle.py, numpy,
    complex step -- not the product's dynamics.hpp); script settings (rti, rti_steps, weights, E): pendulum rti=3 / 2 fast-SLS steps
    (main_pendulum...:49-58), quadrotor rti=3 / 2 (main_quadrotor...:62-69), rocket rti=1 / 1 (main_rocket...:80-85)."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model
    from problems import run_oracle_closed_loop
    m = get_model(model)
    B = 3
    rng = np.random.default_rng(11)
    x0 = np.stack([m.x_ref + amp * 0.05 * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, m.nx) for _ in range(B)])
    if model == "pendulum":
        x0[0] = m.extra["x0"]          # the script's initial state (main_pendulum...:60)
    if model == "quadrotor":           # the script's recipe for its (unseeded) random initial state, seeded here (main_quadrotor...:82-90)
        D = np.array([2.0] * 3 + [1.0] * 3 + [0.0] + [0.1] * 3 + [0.5] * 3)
        x0 = m.x_ref + D * rng.uniform(-1, 1, (B, m.nx))
        x0[:, 6:10] /= np.linalg.norm(x0[:, 6:10], axis=1, keepdims=True)
    W = rng.uniform(-1, 1, (steps, B, m.nx)) if model == "rocket" else None
    cl = ClosedLoopMPC(m, N, B)
    out = cl.run(x0, steps, W)
    cl.close()
    cl = ClosedLoopMPC(m, N, B)                 # a fresh handle: the QP warm start remembers the previous run's active sets
    dev = cl.run_on_device(x0, steps, W)       # records kept in device buffers, one read-back at the end: same bits
    cl.close()
    for k in ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x",
              "backoff_trajectory_u", "success", "scp_iterations"):
        assert np.array_equal(out[k], dev[k]), k
    for b in range(B):
        ref = run_oracle_closed_loop(m, N, x0[b], steps, m.rti, m.fast_sls_rti_steps, None if W is None else W[:, b])
        assert list(out["success"][b]) == list(ref["success"])
        scale = max(1.0, np.abs(ref["nominal_x"]).max())
        assert np.max(np.abs(out["state_trajectory"][b].T - ref["state"])) < 1e-6 * scale
        assert np.max(np.abs(out["input_trajectory"][b].T - ref["u0"][: steps - 1])) < 1e-6 * max(1.0, np.abs(ref["u0"]).max())
        assert np.max(np.abs(out["nominal_trajectory_x"][b].transpose(2, 1, 0) - ref["nominal_x"])) < 1e-6 * scale
        for i in range(steps):
            if ref["backoff_x"][i] is not None:
                assert np.allclose(out["backoff_trajectory_x"][b][:, :, i].T, ref["backoff_x"][i], rtol=1e-5, atol=1e-8)
        # primal_infeasibility of socp_step (SCP_SLS_jit.py:449-456): O(linearisation error^2), compared absolutely
        ok = np.array(ref["success"], dtype=bool)
        assert np.allclose(out["primal_infeasibility"][b][ok], np.array(ref["primal_infeasibility"])[ok], rtol=1e-4, atol=1e-9)
        assert np.array_equal(out["primal_infeasibility"][b], dev["primal_infeasibility"][b], equal_nan=True)
    assert (out["t_jac"] > 0).all() and (dev["t_jac"] > 0).all()      # the linearisation is timed on the device (the scripts' t_jac)


@pytest.mark.parametrize("model,N,steps,sls_steps,amp,scp_eps", [("pendulum", 10, 2, None, 0.04, 1e-8), ("pendulum", 10, 2, 2, 0.04, 1e-8),
                                                                 ("quadrotor", 20, 1, 1, 0.04, 1e-8), ("rocket", 20, 1, 1, 0.01, 1e-6),
                                                                 ("rocket", 20, 1, None, 0.01, 1e-6)])
def test_closed_loop_scp_converge_mode_vs_oracle(model, N, steps, sls_steps, amp, scp_eps):
    """SCP_SLS's default rti = -1 (BASELINE config 4, "full SCP_SLS_jit outer loop"): every instance iterates linearise -> fast-SLS ->
    nominal += delta until |delta|inf < epsilon_convergence, leaving the loop on its own (SCP_SLS_jit.py:113-135); inner fast-SLS in
    converge mode (sls_steps None, MAX_ITER 30) or RTI.  The rocket cases are BASELINE config 4 itself (rockETH N=20, SCP outer loop).
    epsilon_convergence is loosened from the reference's 1e-10 on BOTH sides: the last digits of a QP solution are solver noise (1e-9 relative),
    and the test compares iteration counts.  The rocket starts 1 % of the box away from hover: from 2-4 % some of these random states make the
    SCP iteration expansive (steps of order 1; differences of 1e-8 between two exact QP solvers grow tenfold per iteration) or drive the
    oracle's ADMM restatement to its 50 000-iteration cap on the tightened QP (scripts/diag_rocket_converge.py, diag_inner_converge.py)."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model
    from problems import run_oracle_closed_loop
    m = get_model(model)
    B = 3
    rng = np.random.default_rng(23)
    x0 = np.stack([m.x_ref + amp * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, m.nx) for _ in range(B)])
    cl = ClosedLoopMPC(m, N, B, rti=-1, fast_sls_rti_steps=sls_steps)
    cl.f.opts.scp_eps = scp_eps
    out = cl.run(x0, steps, None)
    kkt = cl.f.get("kkt", (8,))
    cl.close()
    compared = 0
    for b in range(B):
        ref = run_oracle_closed_loop(m, N, x0[b], steps, -1, sls_steps, None, scp_eps=scp_eps)
        if not all(ref["oracle_qp_converged"]):
            # the oracle's ADMM hit its iteration cap on a QP whose outcome fast_SLS.solve ignores: its trajectory is not the exact one
            # (scripts/diag_inst1.py).  Same loop again with the QPs solved by the dense interior point of tests/ref_ipm.py instead.
            ref = run_oracle_closed_loop(m, N, x0[b], steps, -1, sls_steps, None, scp_eps=scp_eps, qp_backend="ipm")
            assert kkt[b, :3].max() < 1e-8
        compared += 1
        assert list(out["success"][b]) == list(ref["success"])
        assert list(out["scp_iterations"][b]) == list(ref["scp_iterations"])
        scale = max(1.0, np.abs(ref["nominal_x"]).max())
        assert np.max(np.abs(out["nominal_trajectory_x"][b].transpose(2, 1, 0) - ref["nominal_x"])) < 1e-6 * scale
        assert np.max(np.abs(out["nominal_trajectory_u"][b].transpose(2, 1, 0) - ref["nominal_u"])) < 1e-6 * max(1.0, np.abs(ref["nominal_u"]).max())
    assert compared >= 2
    assert out["scp_iterations"].max() >= 2          # the loop really iterated


@pytest.mark.parametrize("model,B", [("quadrotor", 64), ("rocket", 32)])
def test_mixed_precision_matches_fp64_and_oracle(model, B):
    """BASELINE config 3 ("fp32 vs fp64"): opts.precision = 1 runs the block factorisations, the stored inverses and the substitutions
    in fp32 and keeps right-hand sides, residuals and the KKT certificate in fp64 (mixed-precision iterative refinement).  Because the
    certificate is fp64, a certified result must agree with the fp64 solver to the same 1e-6 the fp64 path is held to -- for every
    interior-point tolerance of the sweep -- and with the CPU oracle."""
    from robust_nonlinear_mpc_amd import make_batch
    batch = make_batch(model, os.path.join(GOLDEN, {"quadrotor": "sweep_quadrotor_N20_s0.npz", "rocket": "sweep_rocket_N20_s0.npz"}[model]), B, seed=7)
    m, N = batch["model"], batch["N"]
    from robust_nonlinear_mpc_amd import BatchedFastSLS
    f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=B)
    f.update_dynamics_list(batch["A"], batch["B"], batch["E"], batch["g"], batch["gN"], batch["c"])
    f.update_linear_cost(batch["q"])
    x0 = batch["x0_arg"]
    ub, lb = f.get("ubg", (f.mb,)), f.get("lbg", (f.mb,))
    l = np.concatenate([lb, -x0 - 1e-10], axis=1)
    u = np.concatenate([ub, -x0 + 1e-10], axis=1)
    f.qp_update_data_vec(batch["q"], l, u)
    f.opts.warm_start = 0
    f.opts.precision, f.opts.qp_eps = 0, 1e-9
    xr, yr, st, it, _ = f.qp_solve()
    assert (st == 0).all()
    for eps in (1e-3, 1e-5, 1e-6, 1e-9):
        f.opts.precision, f.opts.qp_eps = 1, eps
        f.kernel_timing()
        x, y, st, it, _ = f.qp_solve()
        f.kernel_timing()
        kk = f.get("kkt", (8,))
        assert (st == 0).all(), (eps, np.bincount(st))
        assert kk[:, :3].max() < 1e-8 * max(1.0, np.abs(batch["q"]).max())
        for b in range(B):
            assert relerr(x[b], xr[b]) < 1e-6, (eps, b, relerr(x[b], xr[b]))
            assert relerr(y[b], yr[b]) < 1e-5 * max(1.0, np.abs(yr[b]).max()), (eps, b)
    # two instances against the independent CPU solver (OSQP-class restatement driven to 1e-9)
    from oracle import oracle as O
    d = O.dims_of(m.nx, m.nu, m.nw, N, m.ni, m.ni_f)
    for b in range(2):
        xo, yo, info = O.qp_solve(d, batch["A"][b], batch["B"][b], m.G, m.Gf, m.Q, m.R, m.Qf, batch["q"][b], np.maximum(l[b], -1e20), np.minimum(u[b], 1e20),
                                  O.tight_settings())
        assert info.status in (1, 2)
        assert relerr(x[b], xo) < 1e-6
    f.close()


@pytest.mark.parametrize("model,B", [("quadrotor", 2048), ("rocket", 4096)])
def test_mixed_precision_tolerance_sweep_at_baseline_batch_sizes(model, B):
    """BASELINE config 3 at its own sizes (quadrotor B=2048, rocket B=4096, N=20): fp32 factorisations against fp64 for the loosest and a tight
    interior-point tolerance of the sweep; every instance certified by the fp64 KKT certificate and equal to the fp64 result to 1e-6."""
    from robust_nonlinear_mpc_amd import BatchedFastSLS, make_batch
    batch = make_batch(model, os.path.join(GOLDEN, {"quadrotor": "sweep_quadrotor_N20_s0.npz", "rocket": "sweep_rocket_N20_s0.npz"}[model]), B, seed=3)
    m, N = batch["model"], batch["N"]
    f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=B)
    f.update_dynamics_list(batch["A"], batch["B"], batch["E"], batch["g"], batch["gN"], batch["c"])
    f.update_linear_cost(batch["q"])
    x0 = batch["x0_arg"]
    ub, lb = f.get("ubg", (f.mb,)), f.get("lbg", (f.mb,))
    f.qp_update_data_vec(batch["q"], np.concatenate([lb, -x0 - 1e-10], axis=1), np.concatenate([ub, -x0 + 1e-10], axis=1))
    f.opts.warm_start = 0
    f.opts.precision, f.opts.qp_eps = 0, 1e-9
    xr, yr, st, _, _ = f.qp_solve()
    assert (st == 0).all()
    qn = max(1.0, np.abs(batch["q"]).max())
    for eps in (1e-3, 1e-6):
        f.opts.precision, f.opts.qp_eps = 1, eps
        x, y, st, _, _ = f.qp_solve()
        kk = f.get("kkt", (8,))
        assert (st == 0).all(), (eps, np.bincount(st))
        assert kk[:, :3].max() < 1e-8 * qn
        err = np.abs(x - xr).max(axis=1) / np.maximum(1e-300, np.abs(xr).max(axis=1))
        assert err.max() < 1e-6, (eps, int(err.argmax()), err.max())
        assert (np.abs(y - yr).max(axis=1) < 1e-5 * np.maximum(1.0, np.abs(yr).max(axis=1))).all()
    f.close()


def test_osqp_generated_stand_in_module():
    """Level-2 switch: the module-level singleton the reference drives as `osqp_generated`
    (QP._cg_push_updates qp_jit.py:671-698, QP.solve :449-470): update_data_mat(P_x=, A_x=) -> 0, update_data_vec(q, l, u) -> 0,
    solve() -> (x, y, status_code, iter, run_time) with status_code 0 = solved; data in the reference's frozen CSC order."""
    import scipy.sparse as sp
    from oracle import oracle as O
    from robust_nonlinear_mpc_amd import osqp_generated as cg
    inst = make_instance("pendulum", 2, 1.0)
    m, N = inst.m, inst.N
    nx, nu, nz, ni, nif = m.nx, m.nu, m.nz, m.ni, m.ni_f
    n = nz * N + nx
    # constraint matrix exactly as QP._assemble_structures lays it out (qp_jit.py:101-123, 178-186), dense A_k, B_k blocks
    rows = []
    for k in range(N):
        r = np.zeros((nx, n)); r[:, k * nz:k * nz + nx] = inst.A[k]; r[:, k * nz + nx:(k + 1) * nz] = inst.B[k]; r[:, (k + 1) * nz:(k + 1) * nz + nx] = -np.eye(nx)
        gk = np.zeros((ni, n)); gk[:, k * nz:(k + 1) * nz] = m.G
        rows += [r, gk]
    gf = np.zeros((nif, n)); gf[:, N * nz:] = m.Gf
    pin = np.zeros((nx, n)); pin[:, :nx] = np.eye(nx)
    Amat = np.vstack(rows + [gf, pin])
    # frozen pattern: dense A_k, B_k (incl. zeros), the -I, G, Gf and pin entries
    mask = (Amat != 0)
    for k in range(N):
        mask[k * (nx + ni):k * (nx + ni) + nx, k * nz:(k + 1) * nz] = True
    A_csc = sp.csc_matrix((Amat[mask.nonzero()], mask.nonzero()), shape=Amat.shape)
    A_csc.sort_indices()
    Hd = np.concatenate([np.concatenate([np.diag(m.Q), np.diag(m.R)])] * N + [np.diag(m.Qf)])
    P_ut = sp.triu(sp.diags(2.0 * Hd), format="csc")
    l, u = qp1_bounds(inst)
    assert cg.update_data_mat(P_x=P_ut.data, A_x=A_csc.data) == 0
    assert cg.update_data_vec(inst.q, l, u) == 0
    x, y, status_code, iters, run_time = cg.solve()
    assert status_code == 0 and run_time > 0 and x.shape == (n,) and y.shape == (Amat.shape[0],)
    xo, yo, info = O.qp_solve(oracle_dims(inst), inst.A, inst.B, m.G, m.Gf, m.Q, m.R, m.Qf, inst.q, l, u, O.tight_settings())
    assert relerr(x, xo) < 1e-6
    assert np.abs(Amat[-nx:] @ x - 0.5 * (l[-nx:] + u[-nx:])).max() < 1e-9          # x0 pin rows honoured
    # second solve with new vectors only (the reference pushes vectors every solve)
    assert cg.update_data_vec(0.5 * inst.q, l, u) == 0
    x2 = cg.solve()[0]
    assert relerr(x2, x) > 1e-4
    cg.reset()


def test_drop_in_surface_with_a_reference_shaped_ltv_object():
    """Level-1 switch: SCP_SLS builds `fast_SLS(N, Q, R, LTV(m, N), Qf)` from an object that only has what
    dyn/LTV.py:17-32 copies from the plant, assigns `.Q_reg/.R_reg/.Q_reg_f` afterwards (SCP_SLS_jit.py:386-388), reads
    `.solver_forward.P_mat_csc` (:389) and `.solver_forward.ubg` (:86, :521), calls `.solver_forward.update_ubg` (:99) and the scripts set
    `.solver_forward.verbose / .export_standard_qp` (expe/main_rocket...:86-91).  All of that must work and mean the same."""
    from robust_nonlinear_mpc_amd import fast_SLS
    inst = make_instance("pendulum", 1, 0.5)
    m, N = inst.m, inst.N

    class LTVLike:                               # dyn/LTV.py:17-32
        pass
    ltv = LTVLike()
    ltv.N, ltv.nx, ltv.nu, ltv.nw, ltv.G, ltv.ni, ltv.Gf, ltv.gf, ltv.ni_f = N, m.nx, m.nu, m.nw, m.G, m.ni, m.Gf, m.gf, m.ni_f

    f = fast_SLS(N, m.Q, m.R, ltv, m.Qf)         # regularisers default to identity (ocp.py:14-27)
    f.Q_reg, f.R_reg, f.Q_reg_f = m.Q_reg, m.R_reg, m.Q_reg_f
    f.solver_forward.verbose = False
    f.solver_forward.export_standard_qp = False
    f.set_rti_steps(1)
    P = f.solver_forward.P_mat_csc
    Hd = np.concatenate([np.concatenate([np.diag(m.Q), np.diag(m.R)])] * N + [np.diag(m.Qf)])
    assert P.shape == (f.n, f.n) and np.allclose(P.diagonal(), Hd) and abs(P - P.T).max() == 0
    f.update_dynamics_list(list(inst.A), list(inst.B), list(inst.E), inst.g_list, list(inst.c))
    f.update_linear_cost(0.5 * inst.q)
    f.add_linear_cost(0.5 * inst.q)
    out = f.solve(inst.x0_arg)
    ref = run_oracle_fastsls(inst, rti_steps=1)
    assert out["success"] and relerr(out["primal_vec"], ref["primal_vec"]) < 1e-6
    assert relerr(out["backoff"], ref["backoff"]) < 1e-6          # needs the assigned regularisers, not the identity defaults
    ubg = np.array(f.solver_forward.ubg, dtype=float).reshape(-1)   # the tightened bounds of the last step (SCP_SLS_jit.py:521)
    assert ubg.shape == (f.mb,)
    # update_ubg: closing the first input's box to a single point must pin that input in the next QP
    f.update_dynamics_list(list(inst.A), list(inst.B), list(inst.E), inst.g_list, list(inst.c))
    f.update_linear_cost(inst.q)
    ub = np.array(f.solver_forward.ubg, dtype=float).reshape(-1)
    SR = m.nx + m.ni
    target = 0.25 * ub[m.nx + m.nx]                                  # inside the box of u_0
    ub2 = ub.copy()
    ub2[m.nx + m.nx] = target                                        # u_0 <= target
    ub2[m.nx + m.nz + m.nx] = -target                                # -u_0 <= -target
    f.solver_forward.update_ubg(ub2)
    x, y, st, it, _ = f.qp_solve()
    assert st[0] == 0 and abs(x[0, m.nx] - target) < 1e-8
    f.close()


def test_sliced_batch_is_bitwise_the_single_slice_result():
    """bench.py / Monte-Carlo runs cut a rank's batch into independent slices (own handle, stream and host thread each) that advance
    without lockstep.  An instance is always computed by one wavefront from its own data, so slicing must not change a single bit."""
    from robust_nonlinear_mpc_amd import BatchedFastSLS, make_batch
    from robust_nonlinear_mpc_amd.fast_sls import SlicedDeviceBatch
    B = 96
    batch = make_batch("quadrotor", os.path.join(GOLDEN, "sweep_quadrotor_N20_s0.npz"), B, seed=3)
    m, N = batch["model"], batch["N"]

    def make_solver(nb):
        f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=nb)
        f.set_rti_steps(1)
        f.opts.warm_start = 0
        f.opts.time_kernels = 1          # per-launch HIP events are opt-in (bench.py's roofline leg)
        return f

    res = {}
    for K in (1, 3):
        dev = SlicedDeviceBatch(make_solver, batch, K)
        acc = dev.run(2)
        assert len(acc) == K and all(a["qp"] > 0 for a in acc)
        res[K] = {k: dev.get(k, shp) for k, shp in (("primal_vec", (dev.solvers[0].n,)), ("dual_vec", (dev.solvers[0].mb,)), ("backoff", (N, m.ni)))}
        res[K]["status"] = dev.get("status", (), np.int32)
        ms, launches, sweeps, _ = dev.kernel_timing()
        assert launches > 0 and sweeps >= launches
        dev.close()
    assert (res[1]["status"] == 0).all()
    for k in res[1]:
        assert np.array_equal(res[1][k], res[3][k]), k


def _nlp_kkt_residual(m, N, X, U, x_meas):
    """Independent certificate for the nominal NLP (solver/nlp.py:158-217): dynamics defect, box violation, and the stationarity
    residual min over multipliers (nu free, lambda >= 0 on active bounds only) of |2 H y + J' nu + sum_active +-lambda|."""
    from scipy.optimize import lsq_linear
    from problems import host_ddyn, host_jac
    nx, nu, nz, mid = m.nx, m.nu, m.nz, m.model_id
    n = nz * N + nx
    y = np.concatenate([np.concatenate([X[k], U[k]]) for k in range(N)] + [X[N]])
    Hd = np.concatenate([np.concatenate([np.diag(m.Q), np.diag(m.R)])] * N + [np.diag(m.Qf)])
    hi = np.concatenate([np.concatenate([m.x_ub, m.u_ub])] * N + [m.x_ub])
    lo = np.concatenate([np.concatenate([m.x_lb, m.u_lb])] * N + [m.x_lb])
    J = np.zeros((nx * (N + 1), n))
    J[:nx, :nx] = np.eye(nx)
    defect = 0.0
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
    cols = [J.T] + [np.eye(n)[:, act_u], -np.eye(n)[:, act_l]]
    M = np.hstack(cols)
    lb = np.concatenate([-np.inf * np.ones(J.shape[0]), np.zeros(len(act_u) + len(act_l))])
    sol = lsq_linear(M, -2.0 * Hd * y, bounds=(lb, np.inf * np.ones(M.shape[1])), tol=1e-14, max_iter=500)
    stat = np.abs(M @ sol.x + 2.0 * Hd * y).max() / max(1.0, np.abs(2.0 * Hd * y).max())
    return defect, viol, stat, np.abs(X[0] - x_meas).max(), len(act_u) + len(act_l)


@pytest.mark.parametrize("model,N,amp", [("pendulum", 10, 0.2), ("quadrotor", 20, 0.15), ("rocket", 20, 0.2)])
def test_nominal_initialiser_reaches_nlp_kkt_point(model, N, amp):
    """slsqp_nominal_solve (the role of IPOPT in SCP_SLS.solve_nominal_trajectory, SCP_SLS_jit.py:161-188) from the zero-order roll-out:
    every instance must end at a point that satisfies the nominal NLP's KKT conditions, certified here independently of the solver
    (CPU dynamics/Jacobians + a bounded least-squares fit of the multipliers).  No IPOPT output exists offline: parity unpinned."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model
    m = get_model(model)
    B = 6
    x0 = []
    for s in range(B):
        rng = np.random.default_rng(100 + s)
        x = m.x_ref + amp * 0.25 * (m.x_ub - m.x_lb) * rng.uniform(-1, 1, m.nx)
        if model != "pendulum":
            x[6:10] /= np.linalg.norm(x[6:10])
        x0.append(x)
    x0 = np.stack(x0)
    if model == "pendulum":
        x0[0] = m.extra["x0"]
    cl = ClosedLoopMPC(m, N, B)
    cl.reset(x0, solve_nominal=True)
    X, U = cl.f.get("nominal_x", (N + 1, m.nx)), cl.f.get("nominal_u", (N, m.nu))
    st, its, info = cl.nlp_status, cl.nlp_iterations, cl.nlp_info
    # the roll-out itself is far from optimal / feasible for at least one instance, so the solver had work to do
    assert its.max() >= 3
    assert (st == 0).all(), (st, its, info[:, :8])
    nact = 0
    for b in range(B):
        defect, viol, stat, pin, na = _nlp_kkt_residual(m, N, X[b], U[b], x0[b])
        assert defect < 1e-6 and viol < 1e-8 and pin < 1e-12, (b, defect, viol, pin)
        assert stat < 1e-5, (b, stat)
        nact += na
    # and a closed-loop step from the solved nominal works
    r = cl.step(None)
    assert r["success"].all()
    cl.close()


def test_script_rocket_x0_runs_closed_loop_from_the_gpu_initialiser():
    """The rocket script's own initial state (expe/main_rocket_robust_closed_loop.py:110-126: an attitude 75 degrees off, servos deflected) is
    out of reach of a plain roll-out.  With the initial-state continuation of the nominal initialiser the first nominal is a KKT point of the nominal
    NLP (independent certificate: CPU dynamics and Jacobians) and the script's closed loop (rti = 1, one fast-SLS step, N = 15, seed-0 noise) solves
    every MPC step.  IPOPT's own nominal is not available offline: parity unpinned for the trajectory values."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, disturbance_stream, get_model
    from problems import host_ddyn
    m = get_model("rocket")
    N, B, steps = 15, 2, 5
    x0 = np.tile(m.extra["x0"], (B, 1))
    W = np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)
    cl = ClosedLoopMPC(m, N, B)
    cl.reset(x0, solve_nominal=True, continuation=2)
    X, U = cl.f.get("nominal_x", (N + 1, m.nx)), cl.f.get("nominal_u", (N, m.nu))
    assert (cl.nlp_status == 0).all(), (cl.nlp_status, cl.nlp_info[:, :8])
    for b in range(B):
        kdef, kviol, kstat, kpin, _ = _nlp_kkt_residual(m, N, X[b], U[b], x0[b])        # independent KKT certificate of the nominal NLP
        assert kdef < 1e-6 and kviol < 1e-8 and kstat < 1e-5 and kpin < 1e-9, (kdef, kviol, kstat, kpin)
        assert np.abs(X[b, 0] - x0[b]).max() < 1e-9
        defect = max(np.abs(host_ddyn(m.model_id, X[b, k], U[b, k]) - X[b, k + 1]).max() for k in range(N))
        assert defect < 1e-6, defect
        assert (X[b, 1:] <= m.x_ub + 1e-8).all() and (X[b, 1:] >= m.x_lb - 1e-8).all()
        assert (U[b] <= m.u_ub + 1e-8).all() and (U[b] >= m.u_lb - 1e-8).all()
    # the closed loop from that nominal against the CPU restatement started from the SAME first nominal (the role IPOPT's has in the script):
    # states, inputs and nominal trajectories to 1e-6, step by step, with the seeds' own disturbance streams
    from problems import run_oracle_closed_loop
    out = [cl.step(W[i]) for i in range(steps)]
    cl.close()
    assert np.all([o["success"] for o in out])
    for b in range(B):
        # QPs by the dense interior point (tests/ref_ipm.py via problems.ipm_backend): from this initial state the oracle's ADMM restatement does not
        # reach eps 1e-9 within its 50 000 iterations (its first QP already fails); test_host_cpu pins the two back ends against each other
        ref = run_oracle_closed_loop(m, N, x0[b], steps, m.rti, m.fast_sls_rti_steps, W[:, b], X_nom=X[b], U_nom=U[b], qp_backend="ipm")
        assert all(ref["success"])
        scale = max(1.0, np.abs(ref["nominal_x"]).max())
        compared = 0
        for i in range(steps):
            compared += 1
            assert np.max(np.abs(out[i]["nominal_x"][b] - ref["nominal_x"][i])) < 1e-6 * scale, (b, i, ref["oracle_qp_converged"])
            assert np.max(np.abs(out[i]["nominal_u"][b] - ref["nominal_u"][i])) < 1e-6 * max(1.0, np.abs(ref["nominal_u"]).max()), (b, i)
            # back-offs follow the QP's multipliers through eta = mu / (2 sqrt(beta)); the dense interior point's multipliers are good to ~1e-6
            assert np.allclose(out[i]["backoff_x"][b], ref["backoff_x"][i], rtol=1e-4, atol=1e-8)
        assert compared >= 1, ref["oracle_qp_converged"]


def _script_regime_run(m, N, seeds, steps, check_kkt):
    """Closed loop of the rocket script (its own x0, weights, rti = 1 / one fast-SLS step, 30 steps, seed s = the stream of np.random.seed(s)) for
    `seeds`, step by step; returns per-step arrays and, with check_kkt, the independent KKT residuals (oracle/sls_oracle.c so_qp_kkt) of every
    final QP the GPU reports solved."""
    from oracle import oracle as O
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, disturbance_stream
    B = len(seeds)
    W = np.stack([disturbance_stream(s, steps, m.nx) for s in seeds], axis=1)
    cl = ClosedLoopMPC(m, N, B)
    cl.reset(np.tile(m.extra["x0"], (B, 1)), solve_nominal=True, continuation=2)
    assert (cl.nlp_status == 0).all()
    f = cl.f
    n, mb = f.n, f.mb
    d = O.dims_of(m.nx, m.nu, m.nw, N, m.ni, m.ni_f)
    rec = dict(success=[], qp_stats=[], x=[], u0=[], nominal_x=[], kkt_worst=np.zeros(4), kkt_checked=0)
    for i in range(steps):
        cl.step(W[i], fetch=False)
        qs = f.get("qp_stats", (2, 8), np.int32)
        rec["success"].append(f.get("scp_success", (), np.int32).astype(bool)); rec["qp_stats"].append(qs)
        rec["x"].append(f.get("x_meas", (m.nx,))); rec["u0"].append(f.get("u0", (m.nu,))); rec["nominal_x"].append(f.get("nominal_x", (N + 1, m.nx)))
        if check_kkt:
            A, Bm, q = f.get("A", (N, m.nx, m.nx)), f.get("Bm", (N, m.nx, m.nu)), f.get("q", (n,))
            ub, lb, x0a = f.get("ubg", (mb,)), f.get("lbg", (mb,)), f.get("x0_arg", (m.nx,))
            pv, dv, pin, st = f.get("primal_vec", (n,)), f.get("dual_vec", (mb,)), f.get("pin_dual", (m.nx,)), f.get("status", (), np.int32)
            for b in np.flatnonzero((qs[:, 1, 6] == 0) & (st == 0)):      # the tightened QP (the one whose primal is applied) ended certified
                l = np.concatenate([np.maximum(lb[b], -1e20), -x0a[b] - 1e-10]); u = np.concatenate([ub[b], -x0a[b] + 1e-10])
                k = O.qp_kkt(d, A[b], Bm[b], m.G, m.Gf, m.Q, m.R, m.Qf, q[b], l, u, pv[b], np.concatenate([dv[b], pin[b]]))
                scale = max(1.0, np.abs(q[b]).max())
                rec["kkt_worst"] = np.maximum(rec["kkt_worst"], [k["stationarity"] / scale, k["primal"], k["dual_sign"] / scale, k["complementarity"] / scale])
                rec["kkt_checked"] += 1
    cl.close()
    return {k: (np.stack(v) if isinstance(v, list) else v) for k, v in rec.items()}


def test_script_regime_64_seeds_30_steps_every_qp_certified_or_flagged():
    """The reference script's own regime as a tested configuration (expe/main_rocket_robust_closed_loop.py:110-128, 149-182): script x0, N = 20,
    64 disturbance seeds x all 30 closed-loop steps.  Every QP is either certified (status 0; the tightened QP's certificate re-computed on the CPU
    by the oracle's independent KKT routine), flagged infeasible at x0 before any work (status 2), skipped because the step had failed (-1), or
    flagged unsolved (1 / 3) -- the last within the fraction bench.py reports for this regime; the rerun is bit-identical."""
    from robust_nonlinear_mpc_amd import get_model
    m = get_model("rocket")
    N, S, steps = 20, 64, 30
    r1 = _script_regime_run(m, N, np.arange(S), steps, check_kkt=True)
    r2 = _script_regime_run(m, N, np.arange(S), steps, check_kkt=False)
    for k in ("x", "u0", "nominal_x", "success", "qp_stats"):
        assert np.array_equal(r1[k], r2[k]), k
    st = r1["qp_stats"][..., 6]                                    # (steps, S, 2)
    assert np.isin(st, (-1, 0, 1, 2, 3, 4, 5)).all()
    ran = (st != -1) & (st != 2)
    unsolved = ran & ~np.isin(st, (0, 4))
    # bench.py's 30-step line of this regime (profiles/r03): <= 0.3 % of the QPs that ran end without a solution -- nearly all of them tightened QPs
    # that are infeasible although their x0 is inside its box, ended by the interior point's Farkas certificate (status 5) after ~10 iterations;
    # 64 x 30 x 2 = 3840 QPs here, so allow a handful
    assert unsolved.sum() <= max(4, 0.005 * ran.sum()), (int(unsolved.sum()), int(ran.sum()))
    assert (ran & np.isin(st, (1, 3))).sum() <= 2, np.argwhere(ran & np.isin(st, (1, 3)))
    assert (st[ran] != 4).mean() > 0.99                             # solved means certified, not merely interior-point accurate
    assert ran[:, :, 0].mean() > 0.85 and r1["success"].mean() > 0.7, (ran[:, :, 0].mean(), r1["success"].mean())
    # independent certificate of every tightened QP reported certified: stationarity and multiplier signs 1e-8 |q|inf, complementarity 1e-6 |q|inf, primal
    # residual (dynamics rows and boxes, absolute) 1e-6 -- the tolerance the in-kernel certificate allows the dynamics rows
    assert r1["kkt_checked"] > 0.6 * S * steps, r1["kkt_checked"]
    assert (r1["kkt_worst"] < np.array([1e-8, 1e-6, 1e-8, 1e-6])).all(), r1["kkt_worst"]
    assert np.isfinite(r1["x"]).all() and len({r1["x"][-1, s].tobytes() for s in range(S)}) == S      # seeds differ


def test_script_regime_2_seeds_30_steps_vs_cpu_restatement():
    """Seeds 0 (the script's own disturbance stream) and 1, script x0, N = 20, all 30 closed-loop steps against the CPU restatement of the closed
    loop started from the SAME first nominal (the role IPOPT's has in the script), QPs by the dense interior point (tests/ref_ipm.py): measured
    states, applied inputs and nominal trajectories to 1e-6, step by step, success flags equal."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, disturbance_stream, get_model
    from problems import run_oracle_closed_loop
    m = get_model("rocket")
    N, B, steps = 20, 2, 30
    x0 = np.tile(m.extra["x0"], (B, 1))
    W = np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)
    cl = ClosedLoopMPC(m, N, B)
    cl.reset(x0, solve_nominal=True, continuation=2)
    assert (cl.nlp_status == 0).all()
    X, U = cl.f.get("nominal_x", (N + 1, m.nx)), cl.f.get("nominal_u", (N, m.nu))
    out = [cl.step(W[i]) for i in range(steps)]
    cl.close()
    for b in range(B):
        ref = run_oracle_closed_loop(m, N, x0[b], steps, m.rti, m.fast_sls_rti_steps, W[:, b], X_nom=X[b], U_nom=U[b], qp_backend="ipm")
        assert [bool(o["success"][b]) for o in out] == [bool(v) for v in ref["success"]], b
        sx, su = max(1.0, np.abs(ref["nominal_x"]).max()), max(1.0, np.abs(ref["nominal_u"]).max())
        for i in range(steps):
            assert np.max(np.abs(out[i]["nominal_x"][b] - ref["nominal_x"][i])) < 1e-6 * sx, (b, i)
            assert np.max(np.abs(out[i]["nominal_u"][b] - ref["nominal_u"][i])) < 1e-6 * su, (b, i)
            assert np.max(np.abs(out[i]["u0"][b] - ref["u0"][i])) < 1e-6 * su, (b, i)
            if ref["backoff_x"][i] is not None:
                assert np.allclose(out[i]["backoff_x"][b], ref["backoff_x"][i], rtol=1e-4, atol=1e-8), (b, i)
        assert sum(ref["success"]) >= 20, ref["success"]


@pytest.mark.parametrize("model,N", [("pendulum", 10), ("quadrotor", 20)])
def test_script_length_closed_loops_vs_oracle(model, N):
    """The pendulum script's 60 steps from its own x0 (expe/main_pendulum_robust_closed_loop.py:60, 96; rti = 3, two fast-SLS steps, no noise) and the
    quadrotor script's 30 steps (main_quadrotor...:92; its unseeded random x0 drawn here from a seeded generator by the milder recipe of
    test_closed_loop_vs_oracle) at full length, one instance, against the CPU restatement of the closed loop."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model
    from problems import run_oracle_closed_loop
    m = get_model(model)
    steps = m.extra["sim_steps"]
    if model == "pendulum":
        x0 = m.extra["x0"][None]
    else:
        rng = np.random.default_rng(3)
        D = np.array([2.0] * 3 + [1.0] * 3 + [0.0] + [0.1] * 3 + [0.5] * 3)
        x0 = (m.x_ref + D * rng.uniform(-1, 1, m.nx))[None]
        x0[:, 6:10] /= np.linalg.norm(x0[:, 6:10], axis=1, keepdims=True)
    cl = ClosedLoopMPC(m, N, 1)
    out = cl.run_on_device(x0, steps, None)
    cl.close()
    ref = run_oracle_closed_loop(m, N, x0[0], steps, m.rti, m.fast_sls_rti_steps, None)
    if not all(ref["oracle_qp_converged"]):          # the ADMM restatement gave up on a QP: the dense interior point as the oracle's QP back end
        ref = run_oracle_closed_loop(m, N, x0[0], steps, m.rti, m.fast_sls_rti_steps, None, qp_backend="ipm")
    assert list(out["success"][0]) == list(ref["success"]) and all(ref["success"])
    scale = max(1.0, np.abs(ref["nominal_x"]).max())
    assert np.max(np.abs(out["state_trajectory"][0].T - ref["state"])) < 1e-6 * scale
    assert np.max(np.abs(out["input_trajectory"][0].T - ref["u0"][: steps - 1])) < 1e-6 * max(1.0, np.abs(ref["u0"]).max())
    assert np.max(np.abs(out["nominal_trajectory_x"][0].transpose(2, 1, 0) - ref["nominal_x"])) < 1e-6 * scale


def test_fused_rti_chain_is_bitwise_the_separate_launches():
    """opts.fuse_rti: the one-launch RTI chain (k_rti_chain: every wave takes its instance through QP -> eta -> Riccati / propagation -> tightened
    bounds -> QP) against the separate launches (k_qp_solve, k_after_qp, k_sweep_ric1, k_sweep_prop, k_tighten, k_qp_solve): same device functions in
    the same order per instance, so every result array is identical bit for bit -- rocket closed loop from the script's x0 (active-set rounds,
    interior-point fall-backs, steps flagged at x0), 96 seeds x 8 steps, and the fast-SLS result arrays of the last step."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, disturbance_stream, get_model
    m = get_model("rocket")
    N, B, steps = 20, 96, 8
    W = np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)
    res = []
    for fuse in (1, 0):
        cl = ClosedLoopMPC(m, N, B)
        cl.f.opts.fuse_rti = 2 * fuse          # 2: the chain although the batch is small; 0: the separate launches
        cl.reset(np.tile(m.extra["x0"], (B, 1)), solve_nominal=True, continuation=2)
        outs = [cl.step(W[i]) for i in range(steps)]
        f = cl.f
        last = {k: f.get(k, shp, dt) for k, shp, dt in (("primal_vec", (f.n,), np.float64), ("dual_vec", (f.mb,), np.float64), ("eta", (N, N, m.ni), np.float64),
                                                         ("beta", (N, N, m.ni), np.float64), ("beta_f", (N + 1, m.ni_f), np.float64), ("K", (N, N + 1, m.nu, m.nx), np.float64),
                                                         ("backoff", (N, m.ni), np.float64), ("ubg", (f.mb,), np.float64), ("qp_stats", (2, 8), np.int32),
                                                         ("status", (), np.int32), ("success", (), np.int32), ("iteration_number", (), np.int32), ("cost_tube", (), np.float64))}
        t = f.timing_ms()
        cl.close()
        res.append((outs, last, t))
    (o1, l1, t1), (o0, l0, t0) = res
    for i in range(steps):
        for k in ("u0", "x_next", "nominal_x", "nominal_u", "backoff_x", "backoff_u", "success", "status", "primal_infeasibility"):
            assert np.array_equal(o1[i][k], o0[i][k], equal_nan=True), (i, k)
    for k in l1:
        assert np.array_equal(l1[k], l0[k], equal_nan=True), k
    assert (l1["qp_stats"][:, 1, 0] > 0).any() or (l1["qp_stats"][:, 1, 5] > 0).any()      # the loop did real work in the last step
    assert t1["qp"] > 0 and t1["sweep"] > 0 and t0["qp"] > 0 and t0["sweep"] > 0               # both report a QP and a sweep time


@pytest.mark.parametrize("budget_ms,cut_frac", [(0.3, 0.0), (3.0, 0.0), (1e6, 0.0), (0.0, 0.7), (-1.0, 0.0), (-2.0, 0.0)])
def test_decoupled_closed_loop_is_bitwise_the_step_by_step_loop(budget_ms, cut_frac):
    """slsqp_cl_run (instances advance through their MPC steps independently; a chain still running `budget_ms` after its launch started suspends
    itself between two block solves and resumes in the next round) against the step-by-step loop of slsqp_cl_step: per instance the same operations
    in the same order, so every logged array and every per-QP statistic is identical bit for bit -- whether nearly every solve is cut several
    times (0.3 ms), only the slow ones (3 ms), none (the budget never expires: rounds = steps), or the last 30 % of every round's chains (no time
    limit, cut_frac 0.7).  budget_ms < 0 here stands for the PERSISTENT launch (opts.cl_persistent = 1, the default of the library: waves take
    instances from a device-side FIFO and run whole MPC steps, linearisation and plant included, inside one kernel): -1 with as many waves as
    instances, -2 with 7 waves for the 96 instances (SLSQP_LOOP_WAVES: every instance changes hands between waves ten times).
    Rocket from the script's x0, 96 seeds x 10 steps."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, disturbance_stream, get_model
    m = get_model("rocket")
    N, B, steps = 20, 96, 10
    x0 = np.tile(m.extra["x0"], (B, 1))
    W = np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)
    cl = ClosedLoopMPC(m, N, B)
    L = __import__("robust_nonlinear_mpc_amd")._lib
    assert L.load().slsqp_cl_log(cl.f.h, steps) == 0
    cl.reset(x0, solve_nominal=True, continuation=2)
    ref_stats = []
    for i in range(steps):
        cl.step(W[i], fetch=False)
        ref_stats.append(cl.f.get("qp_stats", (2, 8), np.int32))
    ref = cl._log_result(steps, np.zeros((steps, 1)), np.zeros((steps, 1)), np.zeros((steps, 1)))
    ref_final = {k: cl.f.get(k, shp) for k, shp in (("x_meas", (m.nx,)), ("nominal_x", (N + 1, m.nx)), ("nominal_u", (N, m.nu)), ("primal_vec", (cl.f.n,)))}
    cl.close()
    cl = ClosedLoopMPC(m, N, B)
    cl.f.opts.cl_persistent = 1 if budget_ms < 0 else 0
    if budget_ms == -2.0:
        os.environ["SLSQP_LOOP_WAVES"] = "7"
    try:
        out = cl.run_decoupled(x0, steps, W, solve_nominal=True, continuation=2, budget_ms=budget_ms, cut_frac=cut_frac)
    finally:
        os.environ.pop("SLSQP_LOOP_WAVES", None)
    fin = {k: cl.f.get(k, shp) for k, shp in (("x_meas", (m.nx,)), ("nominal_x", (N + 1, m.nx)), ("nominal_u", (N, m.nu)), ("primal_vec", (cl.f.n,)))}
    cl.close()
    for k in ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x", "backoff_trajectory_u", "success",
              "scp_iterations", "primal_infeasibility"):
        assert np.array_equal(out[k], ref[k], equal_nan=True), k
    for k in fin:
        assert np.array_equal(fin[k], ref_final[k], equal_nan=True), k
    assert np.array_equal(out["qp_stats"], np.stack(ref_stats, axis=1))
    if budget_ms < 0:
        ls = out["loop_stats"]
        assert out["rounds"] == 1 and ls["mpc_steps"] == B * steps and ls["waves"] == (7 if budget_ms == -2.0 else B) and ls["busy_ms"] > 0, ls
    else:
        assert out["rounds"] == steps if budget_ms > 1e5 else out["rounds"] > steps, out["rounds"]


@pytest.mark.parametrize("model,N,B,steps", [("pendulum", 10, 200, 12), ("quadrotor", 20, 150, 8)])
def test_persistent_launch_of_the_other_plants_is_bitwise_the_step_by_step_loop(model, N, B, steps):
    """k_cl_loop is instantiated per plant (its linearisation, plant step and warm-start shift are the plant's): pendulum (transcendental tape of 2 values per
    ODE evaluation) and quadrotor (none) in the setting slsqp_cl_run accepts (rti = 1, one fast-SLS step) against one slsqp_cl_step per step, bit for bit."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, disturbance_stream, get_model
    m = get_model(model)
    x0 = np.tile(m.extra["x0"], (B, 1)) if "x0" in m.extra else np.tile(m.x_ref + 0.02 * (m.x_ub - m.x_lb), (B, 1))
    W = np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)
    outs = []
    for persistent in (0, 1):
        cl = ClosedLoopMPC(m, N, B, rti=1)
        cl.f.set_rti_steps(1)
        if persistent:
            out = cl.run_decoupled(x0, steps, W, solve_nominal=True)
            assert out["rounds"] == 1 and out["loop_stats"]["mpc_steps"] == B * steps
        else:
            out = cl.run_on_device(x0, steps, W, solve_nominal=True)
        outs.append(out)
        cl.close()
    for k in ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x", "backoff_trajectory_u", "success",
              "scp_iterations", "primal_infeasibility"):
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k
    assert outs[0]["success"].mean() > 0.5


def test_persistent_launch_at_full_occupancy_is_bitwise_the_step_by_step_loop():
    """The default regime of slsqp_cl_run: more instances (3500) than the GPU holds wavefronts of k_cl_loop (3072), so every wave serves several
    instances through the device-side FIFO, instances change waves (and XCDs) between their MPC steps, and the ones behind the mean keep theirs --
    against one slsqp_cl_step per step for the whole batch, bit for bit (logged trajectories, success flags, per-QP statistics).  Rocket from the
    script's x0, 5 steps."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, disturbance_stream, get_model
    m = get_model("rocket")
    N, B, steps = 20, 3500, 5
    x0 = np.tile(m.extra["x0"], (B, 1))
    W = np.stack([disturbance_stream(s, steps, m.nx) for s in range(B)], axis=1)
    cl = ClosedLoopMPC(m, N, B)
    L = __import__("robust_nonlinear_mpc_amd")._lib
    assert L.load().slsqp_cl_log(cl.f.h, steps) == 0
    cl.reset(x0, solve_nominal=True, continuation=2)
    ref_stats = []
    for i in range(steps):
        cl.step(W[i], fetch=False)
        ref_stats.append(cl.f.get("qp_stats", (2, 8), np.int32))
    ref = cl._log_result(steps, np.zeros((steps, 1)), np.zeros((steps, 1)), np.zeros((steps, 1)))
    cl.close()
    cl = ClosedLoopMPC(m, N, B)
    assert cl.f.opts.cl_persistent == 1      # the library's default
    out = cl.run_decoupled(x0, steps, W, solve_nominal=True, continuation=2)
    cl.close()
    for k in ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x", "backoff_trajectory_u", "success",
              "scp_iterations", "primal_infeasibility"):
        assert np.array_equal(out[k], ref[k], equal_nan=True), k
    assert np.array_equal(out["qp_stats"], np.stack(ref_stats, axis=1))
    ls = out["loop_stats"]
    assert ls["mpc_steps"] == B * steps and ls["waves"] < B and out["rounds"] == 1, ls


def test_config5_shaped_monte_carlo_1024_seeds_30_steps():
    """BASELINE config 5 at its per-GPU size: 1024 disturbance seeds x 30 closed-loop steps of the rocket (N = 20, script weights, rti = 1, one fast-SLS
    step) from the SCRIPT'S OWN initial state (main_rocket...:110-126; nominal by the GPU initialiser's two-stage continuation).  Properties at full size:
    the rerun is bit-identical, seed 0 follows the reference script's own disturbance stream (tests/golden/rocket_noise_seed0.npz: np.random.seed(0),
    w = 2 rand(17) - 1 per step, main_rocket...:30,180), every step of every run is either solved or flagged, solved steps stay inside the box."""
    from robust_nonlinear_mpc_amd import disturbance_stream, get_model, run_monte_carlo
    m = get_model("rocket")
    S, steps, N = 1024, 30, 20
    x0 = m.extra["x0"]
    r1 = run_monte_carlo(m, N, np.arange(S), steps, x0, slices=3, solve_nominal=True, continuation=2)
    r2 = run_monte_carlo(m, N, np.arange(S), steps, x0, slices=3, solve_nominal=True, continuation=2)
    for k in ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "backoff_trajectory_x", "success", "primal_infeasibility"):
        assert np.array_equal(r1[k], r2[k], equal_nan=True), k
    Wg = np.load(os.path.join(GOLDEN, "rocket_noise_seed0.npz"))["W"]
    assert np.array_equal(disturbance_stream(0, steps, m.nx), Wg[:steps])
    # seed 0's plant really saw that stream: x_{t+1} = ddyn(x_t, u_t) + E w_t with the independent numpy plant
    from problems import host_ddyn
    # (the logged state is the nominal's first state, which a solved step pins to the measured state: only pairs of solved steps are plant steps)
    X, U = r1["state_trajectory"][0], r1["input_trajectory"][0]           # (nx, steps), (nu, steps-1)
    succ = r1["success"]
    pairs = [t for t in range(steps - 1) if succ[0, t] and succ[0, t + 1]]
    assert len(pairs) >= 5, succ[0]
    for t in pairs:
        assert np.allclose(X[:, t + 1], host_ddyn(m.model_id, X[:, t], U[:, t]) + m.E @ Wg[t], rtol=0, atol=1e-9)
    # a step is flagged, not solved, when the noise sample (|w|inf <= 1, i.e. |w|2 up to sqrt(17)) carries the measured state past the bound the
    # 2-norm tube was sized for (from the script's x0 the nominal rides the omega_x and v_z bounds: ~10 % of the steps, more towards the end of the
    # manoeuvre); the reference script would carry on the same way (:149-182)
    assert succ.shape == (S, steps) and succ.mean() > 0.7, succ.mean()
    assert np.isfinite(r1["state_trajectory"]).all()
    # a solved step leaves stages 1 .. N-1 of its nominal inside the box (both QPs bound x_k + dx_k there).  Not the terminal stage: the tightened QP
    # bounds dx_N by the RAW gf (quirk q2, fast_SLS_jit.py:524,568), so x_N may sit outside, and after flagged steps -- which shift the nominal and
    # extrapolate its last stage without a solve -- the whole tail may; the reference's loop does the same, the 2-seed comparison pins it
    nx_ok = r1["nominal_trajectory_x"].transpose(0, 3, 2, 1)           # (runs, steps, N+1, nx)
    after_solved = succ.copy(); after_solved[:, 1:] &= succ[:, :-1]
    inner = nx_ok[after_solved][:, 1:N - 1]
    viol = np.maximum(inner - m.x_ub, m.x_lb - inner)
    assert viol.max() <= 1e-6, float(viol.max())
    assert len({r1["state_trajectory"][s].tobytes() for s in range(0, S, 97)}) == len(range(0, S, 97))    # seeds differ


def test_monte_carlo_seeds_and_npz_keys(tmp_path):
    """Seeded closed-loop Monte-Carlo (config 5 shape, tiny): distinct seeds give distinct trajectories, seed streams are
    reproducible run to run, and the npz written for one instance carries the reference's key set (main_rocket...:189-206)."""
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model, run_monte_carlo
    m = get_model("rocket")
    x0 = m.x_ref + 0.3 * 0.05 * (m.x_ub - m.x_lb) * np.random.default_rng(5).uniform(-1, 1, m.nx)
    r1 = run_monte_carlo(m, 20, [0, 1, 2, 0], 3, x0)
    r2 = run_monte_carlo(m, 20, [0, 1, 2, 0], 3, x0)
    assert np.array_equal(r1["state_trajectory"], r2["state_trajectory"])           # deterministic
    assert np.array_equal(r1["state_trajectory"][0], r1["state_trajectory"][3])      # same seed -> same trajectory
    assert not np.allclose(r1["state_trajectory"][0][:, 1:], r1["state_trajectory"][1][:, 1:])
    assert r1["success"].all()
    r3 = run_monte_carlo(m, 20, [0, 1, 2, 0], 3, x0, slices=3)                        # 3 free-running slices: same bits
    r4 = run_monte_carlo(m, 20, [0, 1, 2, 0], 3, x0, slices=2, budget_ms=0.3)         # ... and through slsqp_cl_run with a budget that cuts every solve
    for k in ("state_trajectory", "input_trajectory", "nominal_trajectory_x", "backoff_trajectory_x", "success"):
        assert np.array_equal(r1[k], r3[k]), k
        assert np.array_equal(r1[k], r4[k]), k
    cl = ClosedLoopMPC(m, 20, 1)
    cl.save_npz(str(tmp_path / "run.npz"), {k: v[:1] if isinstance(v, np.ndarray) and v.shape[:1] == (4,) else v for k, v in r1.items()})
    cl.close()
    keys = set(np.load(str(tmp_path / "run.npz")).keys())
    assert keys == {"state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x",
                    "backoff_trajectory_u", "dt", "g", "nx", "nu", "simulation_time_steps", "N", "t_jac", "t_qp", "t_riccati"}


@pytest.mark.parametrize("model", ["pendulum", "quadrotor"])
def test_fastsls_converge_mode_vs_oracle(model):
    """rti_steps <= 0: iterate _step until the primal moves less than 1e-3 (fast_SLS_jit.py:298-312), per-instance stopping."""
    insts = [make_instance(model, s, a) for a in (0.3, 1.0) for s in range(2)]
    out = run_gpu_fastsls(insts, rti_steps=0)
    for b, inst in enumerate(insts):
        ref = run_oracle_fastsls(inst, rti_steps=None)
        assert bool(out["success"][b]) == bool(ref["success"])
        assert out["iteration_number"][b] == ref["iteration_number"]
        assert relerr(out["primal_vec"][b], ref["primal_vec"]) < 1e-6
        assert relerr(out["backoff"][b], ref["backoff"]) < 1e-6


def test_one_infeasible_instance_does_not_fail_the_batch():
    """Instance 1 gets a measured state far outside its stage-0 box: the reference's QP is infeasible for it
    ({'success': False}, qp_jit.py:397-400); the other instances must be unaffected and identical to a clean batch."""
    _one_bad_instance(100.0)


def test_nan_measured_state_is_flagged_not_solved():
    """A NaN measured state (a failed closed-loop run whose plant overflowed) is outside every box too: flagged like instance 1 above,
    never "solved" into a NaN solution that counts as a successful MPC step."""
    _one_bad_instance(np.nan)


def _one_bad_instance(shift):
    insts = [make_instance("pendulum", s, 0.5) for s in range(4)]
    clean = run_gpu_fastsls(insts, rti_steps=1)
    bad = [make_instance("pendulum", s, 0.5) for s in range(4)]
    bad[1].x0_arg = bad[1].x0_arg + shift
    from problems import make_gpu_solver
    f = make_gpu_solver(bad)
    out = run_gpu_fastsls(bad, rti_steps=1, solver=f)
    qs = f.get("qp_stats", (2, 8), np.int32)
    f.close()
    assert not out["success"][1] and out["status"][1] == 2
    # per-QP statistics: the first QP of instance 1 is flagged without a block solve (status 2), its last QP never runs (status -1);
    # the others ran both and certified them (these are the statuses bench.py's `value` counts by)
    assert qs[1, 0, 6] == 2 and qs[1, 0, 1] == 0 and qs[1, 1, 6] == -1
    assert np.all(qs[[0, 2, 3], :, 6] == 0) and np.all(qs[[0, 2, 3], :, 1] >= 1)
    for b in (0, 2, 3):
        assert out["success"][b]
        assert np.array_equal(out["primal_vec"][b], clean["primal_vec"][b])
        assert np.array_equal(out["backoff"][b], clean["backoff"][b])


def test_reference_shaped_single_instance_view():
    """`fast_SLS` (B=1) takes the reference's list arguments and returns the reference's shapes (fast_SLS_jit.py:250-273, 615-643)."""
    from robust_nonlinear_mpc_amd import fast_SLS
    inst = make_instance("quadrotor", 0, 0.5)
    m, N = inst.m, inst.N
    f = fast_SLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f)
    f.set_rti_steps(2)
    f.update_dynamics_list(list(inst.A), list(inst.B), list(inst.E), inst.g_list, [c for c in inst.c])
    f.update_linear_cost(inst.q.reshape(-1, 1))
    sol = f.solve(inst.x0_arg)
    f.close()
    ref = run_oracle_fastsls(inst, rti_steps=2)
    assert sol["primal_x"].shape == (m.nx, N + 1) and sol["primal_u"].shape == (m.nu, N)
    assert sol["dual_mu"].shape == (m.ni, N) and sol["dual_mu_f"].shape == (m.ni_f,)
    assert sol["eta"].shape == (N, N, m.ni) and sol["K"].shape == (N, N + 1, m.nu, m.nx) and sol["K_mat"].shape == (N * m.nu, (N + 1) * m.nx)
    assert sol["backoff_x"].shape == (N + 1, m.nx) and sol["backoff_u"].shape == (N, m.nu)
    assert sol["Phi_x"] is None and np.isnan(sol["cost_tube"])
    assert bool(sol["success"]) == bool(ref["success"])
    assert np.allclose(sol["primal_x"], ref["primal_x"], rtol=1e-6, atol=1e-7)
    assert np.allclose(sol["dual_mu"], ref["dual_mu"], rtol=1e-5, atol=1e-6 * max(1.0, np.abs(ref["dual_mu"]).max()))
    assert np.allclose(sol["K"], ref["K"], rtol=1e-5, atol=1e-7 * max(1.0, np.abs(ref["K"]).max()))


@pytest.mark.parametrize("model,B", [("pendulum", 1024), ("quadrotor", 2048), ("rocket", 4096)])
def test_full_size_batches_properties(model, B):
    """BASELINE.json batch sizes: size-independent properties.  Every instance ends with a KKT certificate (status 0), two runs are
    bit-identical, and an instance's result does not depend on its position in the batch (reverse the batch -> reversed results)."""
    import os
    from robust_nonlinear_mpc_amd import BatchedFastSLS, make_batch
    fx = {"pendulum": "sweep_pendulum_N10_s0.npz", "quadrotor": "sweep_quadrotor_N20_s0.npz", "rocket": "sweep_rocket_N20_s0.npz"}[model]
    batch = make_batch(model, os.path.join(GOLDEN, fx), B, seed=7)
    m, N = batch["model"], batch["N"]

    def run(order):
        f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=B)
        f.set_rti_steps(1)
        f.update_dynamics_list(batch["A"][order], batch["B"][order], batch["E"], batch["g"][order], batch["gN"][order], batch["c"][order])
        f.update_linear_cost(batch["q"][order])
        f.solve(batch["x0_arg"][order], fetch=False)
        r = dict(primal=f.get("primal_vec", (f.n,)), backoff=f.get("backoff", (N, m.ni)), status=f.get("status", (), np.int32),
                 kkt=f.get("kkt", (8,)), success=f.get("success", (), np.int32))
        f.close()
        return r

    ident = np.arange(B)
    r1, r2, r3 = run(ident), run(ident), run(ident[::-1])
    assert (r1["status"] == 0).all() and r1["success"].all()
    scale = max(1.0, np.abs(batch["q"]).max())
    assert r1["kkt"][:, 0].max() < 1e-9 * scale and r1["kkt"][:, 1].max() < 1e-9 * scale and r1["kkt"][:, 2].max() < 1e-9 * scale
    assert np.array_equal(r1["primal"], r2["primal"]) and np.array_equal(r1["backoff"], r2["backoff"])
    assert np.array_equal(r1["primal"], r3["primal"][::-1]) and np.array_equal(r1["backoff"], r3["backoff"][::-1])
    assert (r1["backoff"][:, :, : m.nx] > 0).all()      # tightening really happened


@pytest.mark.parametrize("nx,nu", [(17, 4), (13, 4)])
def test_wave_level_building_blocks(nx, nu):
    """The hand-written single-wave primitives of csrc/wave_la.hpp, each on its own against numpy (fp64, 1e-12 relative): the MFMA block
    products in the operand layouts the kernels use (plain, transposed, 4-row, diag-scaled, accumulate), the fused product pair of the SLS
    propagation, the 2-D Gauss-Jordan SPD inverse and the D_k assembly of the block factorisation."""
    from robust_nonlinear_mpc_amd import _lib
    import ctypes as C
    L = _lib.load()
    rng = np.random.default_rng(nx)
    MM, NB = nx * nx, nx * nu

    def run(which, ins, n_out):
        a = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in ins]))
        out = np.zeros(n_out)
        rc = L.slsqp_selftest(nx, nu, which, a.ctypes.data_as(C.c_void_p), a.size, out.ctypes.data_as(C.c_void_p), n_out)
        assert rc == 0, L.slsqp_last_error()
        return out

    A, Bq, S = rng.normal(size=(nx, nx)), rng.normal(size=(nx, nx)), rng.normal(size=(nx, nx))
    Bm, K, sc = rng.normal(size=(nx, nu)), rng.normal(size=(nu, nx)), rng.uniform(0.1, 2.0, nx)
    close = lambda got, want: np.max(np.abs(got - want)) < 1e-12 * max(1.0, np.abs(want).max())
    assert close(run(0, [A, Bq], MM).reshape(nx, nx), A @ Bq)
    assert close(run(1, [A, Bq], MM).reshape(nx, nx), A.T @ Bq)
    assert close(run(2, [Bm, S], NB).reshape(nu, nx), Bm.T @ S)
    assert close(run(3, [A, Bq, sc], MM).reshape(nx, nx), (A * sc[None, :]) @ Bq)
    assert close(run(4, [Bm, K, A], MM).reshape(nx, nx), A + Bm @ K)
    o = run(5, [K, A, Bq], NB + MM)
    assert close(o[:NB].reshape(nu, nx), K @ Bq) and close(o[NB:].reshape(nx, nx), A @ Bq)
    # SPD inverse: a matrix conditioned like the D_k of the QPs (entries over a few orders of magnitude), lower triangle given
    Mx = rng.normal(size=(nx, nx + 3))
    Y = (Mx @ Mx.T) * np.outer(sc, sc) + 1e-3 * np.eye(nx)
    o = run(6, [np.tril(Y)], MM + 1)
    assert o[MM] == 0.0
    Di = o[:MM].reshape(nx, nx)
    assert np.array_equal(Di, Di.T)
    assert np.max(np.abs(Di @ Y - np.eye(nx))) < 1e-15 * np.linalg.cond(Y) * nx
    assert np.max(np.abs(Di - np.linalg.inv(Y))) < 1e-15 * np.linalg.cond(Y) * nx * np.abs(np.linalg.inv(Y)).max()
    # a matrix that is not positive definite is reported (pivot clamped, flag set)
    Yb = Y.copy(); Yb[nx // 2, nx // 2] = -1.0
    assert run(6, [np.tril(Yb)], MM + 1)[MM] != 0.0
    # the same inverse by the matrix-core Gauss-Jordan sweep (one rank-2 MFMA update per 2x2 pivot), and its block-packed copy: lane (bi >= bj) of
    # the lower-triangular 2x2 block grid holds rows {2bi, 2bi+1} x columns {2bj, 2bj+1}
    T2 = (nx + 1) // 2
    nblk = T2 * (T2 + 1) // 2
    o = run(8, [np.tril(Y)], MM + 1 + 4 * nblk)
    assert o[MM] == 0.0
    Dm = o[:MM].reshape(nx, nx)
    assert np.array_equal(Dm, Dm.T)
    assert np.max(np.abs(Dm @ Y - np.eye(nx))) < 1e-15 * np.linalg.cond(Y) * nx
    assert np.max(np.abs(Dm - Di)) < 1e-15 * np.linalg.cond(Y) * nx * np.abs(Di).max()
    blocks = o[MM + 1:].reshape(nblk, 2, 2)
    lane = 0
    for bi in range(T2):
        for bj in range(bi + 1):
            rows, cols = [2 * bi, min(2 * bi + 1, nx - 1)], [2 * bj, min(2 * bj + 1, nx - 1)]
            assert np.array_equal(blocks[lane], Dm[np.ix_(rows, cols)]), (bi, bj)
            lane += 1
    assert run(8, [np.tril(Yb)], MM + 1 + 4 * nblk)[MM] != 0.0
    # D_k assembly: lower triangle of  M1 A' + B diag(piu) B' - T M1' + diag(d) + delta,  M1 = A diag(pix)
    T = rng.normal(size=(nx, nx)); pix, piu, d = rng.uniform(0.1, 2.0, nx), rng.uniform(0.1, 2.0, nu), rng.uniform(0.1, 2.0, nx)
    M1 = A * pix[None, :]
    want = M1 @ A.T + (Bm * piu[None, :]) @ Bm.T - T @ M1.T + np.diag(d + 1e-13)
    got = run(7, [A, Bm, T, pix, piu, d], MM).reshape(nx, nx)
    assert close(np.tril(got), np.tril(want))


def test_infeasible_box_is_flagged_early_by_the_stagnation_rule():
    """A QP whose x_0 is fine but whose box is empty at one stage (upper bound below the lower one) has no solution: the interior point must end
    flagged -- by its Farkas certificate (status 5) or, failing that, the stagnation rule (1 / 3), never 0 / 4 -- well before qp_max_iter = 60
    iterations, and its neighbours in the batch are untouched."""
    from robust_nonlinear_mpc_amd import BatchedFastSLS, make_batch
    B = 8
    batch = make_batch("quadrotor", os.path.join(GOLDEN, "sweep_quadrotor_N20_s0.npz"), B, seed=5)
    m, N = batch["model"], batch["N"]
    f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=B)
    f.update_dynamics_list(batch["A"], batch["B"], batch["E"], batch["g"], batch["gN"], batch["c"])
    f.update_linear_cost(batch["q"])
    x0 = batch["x0_arg"]
    ub, lb = f.get("ubg", (f.mb,)), f.get("lbg", (f.mb,))
    l = np.concatenate([lb, -x0 - 1e-10], axis=1); u = np.concatenate([ub, -x0 + 1e-10], axis=1)
    f.opts.warm_start = 0
    f.qp_update_data_vec(batch["q"], l, u)
    xr, yr, st, it, _ = f.qp_solve()
    assert (st == 0).all()
    # instance 2: stage 5, state component 1:  z <= hi  and  -z <= -(hi + 0.5)  cannot both hold
    SR, nz = m.nx + m.ni, m.nx + m.nu
    u2 = u.copy()
    row_hi, row_lo = 5 * SR + m.nx + 1, 5 * SR + m.nx + nz + 1
    u2[2, row_lo] = -(u2[2, row_hi] + 0.5)
    f.qp_update_data_vec(batch["q"], l, u2)
    x, y, st, it, _ = f.qp_solve()
    qs = f.get("qp_stats", (2, 8), np.int32)
    f.close()
    assert st[2] in (1, 3, 5) and it[2] < 45, (st[2], it[2])
    assert qs[2, 0, 1] < 110
    ok = [b for b in range(B) if b != 2]
    assert (st[ok] == 0).all() and np.array_equal(x[ok], xr[ok])


def test_python_mirror_under_debug_allocators():
    """Every entry point of the Python mirror that hands a host buffer to the C ABI, once, in a child process whose allocators check their block
    boundaries (glibc MALLOC_CHECK_=3, PYTHONMALLOC=malloc_debug): an undersized buffer aborts the child instead of corrupting a heap silently."""
    import subprocess, sys
    from conftest import ROOT
    env = dict(os.environ, MALLOC_CHECK_="3", PYTHONMALLOC="malloc_debug")
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.join(ROOT, "tests", "abi_memcheck.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "abi_memcheck ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

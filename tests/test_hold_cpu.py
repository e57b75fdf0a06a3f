"""Hold steps (slsqp_cl_hold_step), the part that needs no GPU: the numpy restatement of the policy (tests/hold_ref.py, which tests/test_gpu_hold.py
holds the HIP kernel against) against the reference's own sweep output, its behaviour for an instance without a valid plan, the C ABI's
declaration and its ctypes mirror, and the call's bookkeeping (csrc/cl_hold.hpp) in a stand-alone program under the sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import hold_ref as HR
import sweep_ref as SR
from conftest import GOLDEN, ROOT

FIXTURES = ["sweep_pendulum_N10_s0", "sweep_quadrotor_N8_s3_nw5", "sweep_rocket_N5_s1"]


# ---- 1: the realisation against the reference's sweep output ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("fixture", FIXTURES)
def test_column_realisation_reproduces_phi_x_and_phi_u(fixture, seed):
    """e_{k+1} = A_k e_k + B_k d_k + E_{k+1} w_{k+1}, e_0 = E_0 w_0, with d_k from hold_ref.policy (column 0 admitted: first = 0), for a seeded w in
    the unit box: e_k = sum_j Phi_x[k,j] w_j and d_k = sum_j Phi_u[k,j] w_j to 1e-10 relative (sums of at most 11 x 17 fp64 terms of O(1); the margin
    tests/test_sweep_ref_cpu.py gives the same data).  A, B, E, K are the fixture's, produced by the reference's kernels.  Phi_x, Phi_u are the
    fixture's for the pendulum; the quadrotor's and the rocket's fixtures hold only block norms of them, so theirs come from tests/sweep_ref.py's
    propagate() on the fixture's A, B, E, K (which tests/test_sweep_ref_cpu.py holds to those norms)."""
    g = dict(np.load(os.path.join(GOLDEN, fixture + ".npz")))
    N, nx, nu, nw = (int(g[k]) for k in ("N", "nx", "nu", "nw"))
    A, B, E, K = g["A"], g["B"], g["E"], g["K"]
    if "Phi_x" in g:
        Px, Pu = g["Phi_x"], g["Phi_u"]
    else:
        Px, Pu = (np.asarray(a, dtype=float) for a in SR.propagate(A, B, E, K))
    assert Px.shape == (N + 1, N + 1, nx, nw) and Pu.shape == (N, N + 1, nu, nw)
    w = np.random.default_rng(100 + seed).uniform(-1.0, 1.0, (N + 1, nw))
    xi = np.zeros((N + 1, nx))
    e = E[0] @ w[0]
    got_e, want_e, got_d, want_d = [], [], [], []
    for k in range(N + 1):
        got_e.append(e); want_e.append(sum(Px[k, j] @ w[j] for j in range(k + 1)))
        if k == N:
            break
        d, xi = HR.policy(k, e, xi, A, B, K, first=0)
        got_d.append(d); want_d.append(sum(Pu[k, j] @ w[j] for j in range(k + 1)))
        assert np.allclose(xi[:k + 1].sum(axis=0), e, rtol=0, atol=1e-12 * max(1.0, np.abs(e).max()))      # the columns sum to the deviation
        e = A[k] @ e + B[k] @ d + E[k + 1] @ w[k + 1]
    worst_e, worst_d = SR.relerr(got_e, want_e), SR.relerr(got_d, want_d)      # max-norm error relative to the largest entry of the response itself
    print(fixture, seed, "e", worst_e, "of", np.abs(want_e).max(), "d", worst_d, "of", np.abs(want_d).max())
    assert worst_e < 1e-10 and worst_d < 1e-10, (worst_e, worst_d)
    assert max(np.abs(Pu[k, j] @ w[j]).max() for k in range(N) for j in range(k + 1)) > 1e-6      # the feedback is not trivially zero


def test_pinned_first_column_is_the_device_case():
    """With x_0 pinned (e_0 = 0, column 0 zero) the columns 1..k alone carry the response: first = 1 and first = 0 give the same inputs."""
    g = dict(np.load(os.path.join(GOLDEN, FIXTURES[0] + ".npz")))
    N, nx, nw = int(g["N"]), int(g["nx"]), int(g["nw"])
    A, B, E, K = g["A"], g["B"], g["E"], g["K"]
    w = np.random.default_rng(7).uniform(-1.0, 1.0, (N + 1, nw))
    xa, xb = np.zeros((N + 1, nx)), np.zeros((N + 1, nx))
    e = E[1] @ w[1]
    for k in range(1, N):
        da, xa = HR.policy(k, e, xa, A, B, K, first=0)
        db, xb = HR.policy(k, e, xb, A, B, K)
        assert np.array_equal(da, db) and np.array_equal(xa, xb) and not xb[0].any() and not xb[k + 1:].any()
        e = A[k] @ e + B[k] @ da + E[k + 1] @ w[k + 1]


# ---- 2: an instance without a valid plan ---------------------------------------------------------------------------------------------------------
def test_failed_instance_applies_the_nominal_input_and_keeps_its_columns():
    g = dict(np.load(os.path.join(GOLDEN, FIXTURES[0] + ".npz")))
    N, nx, nu = int(g["N"]), int(g["nx"]), int(g["nu"])
    rng = np.random.default_rng(3)
    xi = rng.normal(size=(N + 1, nx))
    keep = xi.copy()
    d, new = HR.policy(2, rng.normal(size=nx), xi, g["A"], g["B"], g["K"], hold_policy=0)
    assert not d.any() and np.array_equal(new, keep) and np.array_equal(xi, keep)
    x, z, v = np.array([0.1, 0.0, 0.05, 0.0]), np.array([0.08, 0.0, 0.04, 0.0]), np.array([0.3])
    u, xp, new = HR.hold_step(0, 2, x, z, v, xi, g["A"], g["B"], g["K"], hold_policy=0)
    from oracle import dyn_oracle as DO
    assert np.array_equal(u, v) and np.array_equal(new, keep) and np.array_equal(xp, DO.ddyn(0, x, v))
    u1, _, new1 = HR.hold_step(0, 2, x, z, v, xi, g["A"], g["B"], g["K"])
    assert not np.array_equal(u1, v) and not np.array_equal(new1, keep)      # (the same call with a valid plan does act)


# ---- 3: header and mirror ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_hold_step_and_the_loader_binds_it():
    from robust_nonlinear_mpc_amd import _lib
    text = open(os.path.join(ROOT, "include", "slsqp.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+slsqp_cl_hold_step\s*\(([^)]*)\)\s*;", header)
    assert decl, "slsqp_cl_hold_step is not declared in include/slsqp.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 3 and args[0].startswith("slsqp_handle") and args[1].split() == ["const", "double", "*w"] and args[2].split() == ["int", "loc"], args
    assert "slsqp_cl_hold_step" in _lib.EXPORTS
    for name in ("hold_index", "hold_xi", "hold_policy", "log_hold"):      # the result names are part of the documented interface
        assert re.search(r"\b" + name + r"\b", text), name
    import ctypes
    assert ctypes.sizeof(_lib.Opts) == 104      # how often a solve happens is the caller's choice: slsqp_opts keeps its layout
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert lib.slsqp_cl_hold_step.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]


def test_python_surface_takes_solve_every():
    import inspect
    from robust_nonlinear_mpc_amd import BatchedFastSLS, ClosedLoopMPC, run_monte_carlo
    assert inspect.signature(ClosedLoopMPC.__init__).parameters["solve_every"].default == 1
    for fn in (ClosedLoopMPC.run, ClosedLoopMPC.run_on_device, ClosedLoopMPC.run_decoupled):
        assert inspect.signature(fn).parameters["solve_every"].default is None      # (None: the constructor's)
    assert inspect.signature(run_monte_carlo).parameters["solve_every"].default == 1
    assert callable(BatchedFastSLS.hold_step) and callable(ClosedLoopMPC.hold_step)


# ---- the call's bookkeeping ----------------------------------------------------------------------------------------------------------------------
def test_hold_bookkeeping_under_sanitizers():
    """csrc/cl_hold.hpp (free of HIP calls) in a stand-alone program with its own main, built with -fsanitize=address,undefined: the hold index
    through solve / hold sequences, and every refusal of slsqp_cl_hold_step that does not need a device (no solve yet, the N-th hold in a row, after
    a persistent run, no model, loc), each leaving the state as it was."""
    exe = os.path.join(ROOT, "tests", "_build", "cl_hold_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-o", exe, os.path.join(ROOT, "tests", "cl_hold_check_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cl_hold_check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

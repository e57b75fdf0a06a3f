"""Helpers shared by tests/test_plant_params_cpu.py and tests/test_gpu_plant_params.py (test infrastructure, CPU only).

  * `paramlib()`: tests/dyn_host_params.cpp built by g++ -- csrc/dynamics.hpp on the host with the pointer parameter source (dynp_*) and, from the
    same build, the constant instantiation (dync_*).  The CPU tests pin it to the reference's values with changed parameters; the GPU tests then use
    it as the host's ddyn_p.
  * `pendulum_ode` / `pendulum_ddyn`: a numpy statement of the cart-pole with (m1, m2, l, g).  The reference keeps the pendulum's constants local to
    its ode, so there is no reference value with changed parameters; this statement is first held to tests/golden/dyn_pendulum*.npz at the default
    parameters and then stands in for the reference.
  * `run_oracle_closed_loop_plant`: the CPU closed loop of tests/problems.py whose plant step is a caller's function (the controller keeps the
    numpy restatement of the model).
"""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from problems import host_ddyn, host_jac

NAMES = ("pendulum", "quadrotor", "rocket")
RK4_H = 0.05


def paramlib():
    so = os.path.join(ROOT, "tests", "_build", "libdyn_host_params.so")
    src = os.path.join(ROOT, "tests", "dyn_host_params.cpp")
    hdr = os.path.join(ROOT, "robust-nonlinear-mpc_amd", "csrc", "dynamics.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _call(fn, mid, x, u, p=None):
    x, u = np.ascontiguousarray(x, dtype=float), np.ascontiguousarray(u, dtype=float)
    o = np.zeros_like(x)
    if p is None:
        fn(mid, _p(x), _p(u), _p(o))
    else:
        p = np.ascontiguousarray(p, dtype=float)
        fn(mid, _p(x), _p(u), _p(p), _p(o))
    return o


def host_ode_p(mid, x, u, p):
    return _call(paramlib().dynp_ode, mid, x, u, p)


def host_ddyn_p(mid, x, u, p):
    return _call(paramlib().dynp_ddyn, mid, x, u, p)


def host_ode_c(mid, x, u):
    return _call(paramlib().dync_ode, mid, x, u)


def host_ddyn_c(mid, x, u):
    return _call(paramlib().dync_ddyn, mid, x, u)


def host_defaults(mid):
    lib = paramlib()
    o = np.zeros(lib.dynp_count(mid))
    lib.dynp_defaults(mid, _p(o))
    return o


def pendulum_ode(x, u, p):
    """Cart (mass m1) with a point-mass pole (m2, length l) hinged on it, angle measured from the upright position, force u on the cart."""
    m1, m2, l, g = (float(v) for v in p)
    _, v, th, om = (float(a) for a in x)
    f = float(np.ravel(u)[0])
    s, c = np.sin(th), np.cos(th)
    inertia = m1 + m2 * s * s
    centrifugal = m2 * l * om * om * s
    acc = (f + centrifugal - m2 * g * s * c) / inertia
    alpha = ((m1 + m2) * g * s - f * c - centrifugal * c) / (l * inertia)
    return np.array([v, acc, om, alpha])


def pendulum_ddyn(x, u, p, h=RK4_H):
    x = np.asarray(x, dtype=float)
    k1 = pendulum_ode(x, u, p)
    k2 = pendulum_ode(x + 0.5 * h * k1, u, p)
    k3 = pendulum_ode(x + 0.5 * h * k2, u, p)
    k4 = pendulum_ode(x + h * k3, u, p)
    return x + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)


def spread_params(model, B, pct, seed):
    """(B,np): every parameter of every instance uniform within +-pct % of its default, the gimbal lengths kept: the examples' own sampler, instance
    b drawn from the generator of seed 1000 seed + b."""
    from robust_nonlinear_mpc_amd._plant_cli import sample_plant_params
    return sample_plant_params(model, 1000 * seed + np.arange(B), pct)


def run_oracle_closed_loop_plant(m, N, x0, steps, rti, sls_steps, plant_step):
    """tests/problems.py::run_oracle_closed_loop (zero-order roll-out initialiser, reset_warm_start, tight oracle settings, no noise) with the plant
    update x <- plant_step(x, u0); everything the controller does (roll-out, shift, linearisation) keeps the numpy restatement of the model."""
    from oracle import oracle as O
    d = O.dims_of(m.nx, m.nu, m.nw, N, m.ni, m.ni_f)
    E = np.stack([m.E] * (N + 1))
    fs = O.OracleFastSLS(d, m.G, m.Gf, m.g, m.gf, E, m.Q, m.R, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, O.tight_settings())
    fs.set_rti_steps(sls_steps)
    mid = m.model_id
    X = np.zeros((N + 1, m.nx)); U = np.tile(m.u_ref, (N, 1))
    X[0] = x0
    for k in range(N):
        X[k + 1] = host_ddyn(mid, X[k], U[k])
    Hd = np.concatenate([np.concatenate([np.diag(m.Q), np.diag(m.R)])] * N + [np.diag(m.Qf)])
    xm = np.asarray(x0, dtype=float).copy()
    log = dict(state=[], u0=[], nominal_x=[], nominal_u=[], success=[], oracle_qp_converged=[], model_error=[])
    for i in range(steps):
        if i > 0:
            xN = host_ddyn(mid, X[N], U[N - 1])
            X[:N] = X[1:N + 1].copy(); U[:N - 1] = U[1:N].copy(); X[N] = xN
            fs.reset_solver_to_zeros()
        ok, qp_conv = True, True
        for ii in range(rti):
            A = np.zeros((N, m.nx, m.nx)); Bm = np.zeros((N, m.nx, m.nu)); c = np.zeros((N, m.nx))
            for k in range(N):
                A[k], Bm[k], f = host_jac(mid, X[k], U[k])
                c[k] = f - X[k + 1]
            g_list = [m.g - m.G @ np.concatenate([X[k], U[k]]) for k in range(N)] + [m.gf - m.Gf @ X[N]]
            y_nom = np.concatenate([np.concatenate([X[k], U[k]]) for k in range(N)] + [X[N]])
            fs.update_dynamics_list(A, Bm, E, g_list, c)
            fs.update_linear_cost(2.0 * Hd * y_nom)
            sol = fs.solve(X[0] - xm)
            ok = bool(sol["success"])
            if fs.qp.last_info.status != 1:
                qp_conv = False
            if not ok:
                break
            X = X + sol["primal_x"].T
            U = U + sol["primal_u"].T
        log["oracle_qp_converged"].append(qp_conv)
        log["state"].append(X[0].copy()); log["u0"].append(U[0].copy()); log["nominal_x"].append(X.copy()); log["nominal_u"].append(U.copy())
        log["success"].append(ok)
        xp = np.asarray(plant_step(xm, U[0]), dtype=float)
        log["model_error"].append(xp - host_ddyn(mid, xm, U[0]))
        xm = xp
    return {k: np.array(v) for k, v in log.items()}

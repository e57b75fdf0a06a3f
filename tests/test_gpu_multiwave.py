"""The multi-wave QP path (opts.solve_waves = 2, 4, 8: csrc/slsqp_mw.hpp) against yardsticks that are not the code under test.

1. Linear algebra (slsqp_ne_solve): the block cyclic reduction's nu on corpus systems, horizons 1, 2, 3, 5, 20 (and 64): a root alone, an
   elimination without a right neighbour, odd counts at the first and at a deeper level, more waves than blocks.  Yardsticks: the single-wave
   kernels' sweeps (waves = 1) and the numpy prototype (scripts/proto/cr_normal_eq.py) on the same systems; residuals in long double.
2. QP level: the corpus through slsqp_qp_solve with solve_waves 2 and 8, every host check of tests/test_gpu_qp_paths.py.
3. fast-SLS steps and closed loops against the same runs with one wave; refusals.
"""
import functools
import os
import sys

import numpy as np
import pytest

import qp_corpus as QC
from conftest import ROOT
from problems import make_instance, make_gpu_solver, run_gpu_fastsls
from test_gpu_qp_paths import VARIANTS, _check, _push, _solve, make_gpu_solver_qp

sys.path.insert(0, os.path.join(ROOT, "scripts", "proto"))
import cr_normal_eq as CR  # noqa: E402

pytestmark = pytest.mark.gpu

WAVES = (2, 4, 8)
DELTA = 1e-13
EPS = 2.220446049250313e-16


@functools.lru_cache(maxsize=None)
def _plant(model):
    qps = QC.corpus(model)
    return dict(model=model, qps=qps, refs=[QC.reference(q) for q in qps], lps=[QC.feasibility_margin(q) for q in qps])


# ---- 1. linear algebra ------------------------------------------------------------------------------------------------
def _la_systems(model, N, weighting):
    """three corpus QPs of the plant (an easy one, a stress one, one with a large active set) at the given weighting, the horizon cut to N stages
    (N = 64: the stages behind the first one repeated): A (3,N,nx,nx), B (3,N,nx,nu), PI (3,n)"""
    P = _plant(model)
    pick = []
    for cls in ("easy", "stress", "bigset"):
        pick.append(next((q, r) for q, r in zip(P["qps"], P["refs"]) if q.cls == cls and r is not None))
    A, B, PI = [], [], []
    for qp, ref in pick:
        nz, nx = qp.nz, qp.nx
        # stage k of the cut horizon; past the QP's own horizon its stages 1 .. N-1 repeat (stage 0 is special: x_0 is pinned, its weights are 0)
        idx = np.concatenate([[0], 1 + (np.arange(N) % (qp.N - 1))])
        pi = CR.weighting(qp, CR.active_mask(qp, ref), weighting)
        # (the state weights behind the last stage: the terminal ones for the QP's own horizon, else those of the stage that would follow)
        last = pi[nz * qp.N:] if N == qp.N else pi[nz * idx[N]:nz * idx[N] + nx]
        idx = idx[:N]
        stages = pi[:nz * qp.N].reshape(qp.N, nz)[idx]
        A.append(qp.A[idx]); B.append(qp.B[idx]); PI.append(np.concatenate([stages.ravel(), last]))
    return np.stack(A), np.stack(B), np.stack(PI), pick[0][0].m


def _la_solver(m, N, A, B):
    from robust_nonlinear_mpc_amd import BatchedFastSLS
    Bn = A.shape[0]
    f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=Bn)
    f.update_dynamics_list(A, B, np.stack([m.E] * (N + 1)), np.zeros((Bn, N, m.ni)), np.zeros((Bn, m.ni_f)), np.zeros((Bn, N, m.nx)))
    return f


def _bmax_host(A, B, v):
    """max|b| and the rounding bound of its entries: b_k is a sum of nx + nu + 1 products"""
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    nz = nx + nu
    b = CR.rhs(A, B, v)
    mag = max(float((np.abs(A[k]) @ np.abs(v[k * nz:k * nz + nx]) + np.abs(B[k]) @ np.abs(v[k * nz + nx:(k + 1) * nz]) + np.abs(v[(k + 1) * nz:(k + 1) * nz + nx])).max())
              for k in range(N))
    return b, float(np.abs(b).max()), (nz + 2) * EPS * mag


SHAPES = [(model, N) for model in QC.PLANTS for N in (1, 2, 3, 5, 20)] + [("quadrotor", 64)]


@pytest.mark.parametrize("model,N", SHAPES)
def test_cyclic_reduction_against_sweeps_and_prototype(model, N):
    worst = 0.0
    for weighting in ("active-set", "late-ipm"):
        A, B, PI, m = _la_systems(model, N, weighting)
        Bn, n = A.shape[0], PI.shape[1]
        rng = np.random.default_rng(100 + N)
        V, V2 = rng.normal(size=(Bn, n)), rng.normal(size=(Bn, n))
        sysm = [CR.stage_blocks(A[b], B[b], PI[b], DELTA) for b in range(Bn)]
        host = [[_bmax_host(A[b], B[b], v[b]) for b in range(Bn)] for v in (V, V2)]

        def res(out, which):
            return np.array([CR.residual(sysm[b][0], sysm[b][1], host[which][b][0], out["nu"][b]) for b in range(Bn)])
        f = _la_solver(m, N, A, B)
        try:
            # yardsticks: the single-wave sweeps on the device, the prototype on the host -- for both right-hand sides
            one = [f.ne_solve(PI, V, waves=1, factor=True, delta=DELTA), f.ne_solve(PI, V2, waves=1, factor=False, delta=DELTA)]
            yard = []
            for which in (0, 1):
                proto = np.array([CR.residual(sysm[b][0], sysm[b][1], host[which][b][0], CR.cr(sysm[b][0], sysm[b][1], host[which][b][0])[0]) for b in range(Bn)])
                yard.append(np.maximum(res(one[which], which), proto))
            assert (one[0]["fail"] == 0).all()
            for W in WAVES:
                outs = [f.ne_solve(PI, V, waves=W, factor=True, delta=DELTA), f.ne_solve(PI, V2, waves=W, factor=False, delta=DELTA)]
                for which, (out, v) in enumerate(zip(outs, (V, V2))):
                    tag = f"{model} N={N} {weighting} waves={W} rhs {which}"
                    assert np.isfinite(out["nu"]).all() and np.isfinite(out["G"]).all() and (out["fail"] == 0).all(), tag
                    r = res(out, which)
                    ratio = r / yard[which]
                    print(f"{tag}: residual {r.max():.2e}, yardstick {yard[which].max():.2e}, worst ratio {ratio.max():.2f}")
                    worst = max(worst, float(ratio.max()))
                    assert (ratio <= 4.0).all(), f"{tag}: residuals {r} against {yard[which]}"
                    for b in range(Bn):
                        G = CR.E_t_nu(A[b], B[b], out["nu"][b])
                        assert np.abs(out["G"][b] - G).max() <= 1e-12 * max(np.abs(G).max(), 1e-300), tag
                        assert abs(out["bmax"][b] - host[which][b][1]) <= host[which][b][2], (tag, out["bmax"][b], host[which][b][1])
        finally:
            f.close()
    print(f"{model} N={N}: worst residual ratio against the yardsticks {worst:.2f}")


@pytest.mark.parametrize("model,N,W", [("pendulum", 5, 2), ("rocket", 5, 4), ("quadrotor", 20, 8)])
def test_indefinite_block_is_flagged_and_stays_in_its_instance(model, N, W):
    A, B, PI, m = _la_systems(model, N, "late-ipm")
    V = np.random.default_rng(5).normal(size=PI.shape)
    f = _la_solver(m, N, A, B)
    try:
        clean = f.ne_solve(PI, V, waves=W, delta=DELTA)
        bad = PI.copy()
        bad[1, (N // 2) * (m.nx + m.nu) + m.nx] = -1e6       # an input weight of a middle stage: B diag(pi) B' turns Y_kk indefinite
        out = f.ne_solve(bad, V, waves=W, delta=DELTA)
        assert out["fail"][1] == 1 and out["fail"][0] == 0 and out["fail"][2] == 0, out["fail"]
        for b in (0, 2):
            assert np.array_equal(out["nu"][b], clean["nu"][b]) and np.array_equal(out["G"][b], clean["G"][b])
        assert f.ne_solve(bad, V, waves=1, delta=DELTA)["fail"][1] == 1
    finally:
        f.close()


def test_ne_solve_argument_checks():
    A, B, PI, m = _la_systems("pendulum", 3, "late-ipm")
    f = _la_solver(m, 3, A, B)
    try:
        for W in (0, 3, 16):
            with pytest.raises(RuntimeError, match="waves"):
                f.ne_solve(PI, PI, waves=W)
        with pytest.raises(RuntimeError, match="factor = 0"):
            f.ne_solve(PI, PI, waves=2, factor=False)              # nothing factorised yet
        f.ne_solve(PI, PI, waves=2)
        with pytest.raises(RuntimeError, match="factor = 0"):
            f.ne_solve(PI, PI, waves=4, factor=False)              # the stored factors are another path's
    finally:
        f.close()


# ---- 2. QP level ------------------------------------------------------------------------------------------------------
QP_VARIANTS = ("default", "as_first0", "as_max_viol0", "max_iter8")


def _must_match(P):
    """QPs whose status may not depend on the path: clearly feasible ones (LP margin <= -1e-3) and the four x0-edge QPs"""
    return [b for b, q in enumerate(P["qps"]) if q.cls == "x0edge" or P["lps"][b][0] <= -1e-3]


@pytest.mark.parametrize("W", [2, 8])
@pytest.mark.parametrize("model", QC.PLANTS)
def test_qp_paths_cold_multiwave(model, W):
    P = _plant(model)
    qps, refs, lps = P["qps"], P["refs"], P["lps"]
    f, f1 = make_gpu_solver_qp(qps), make_gpu_solver_qp(qps)
    try:
        f.opts.solve_waves = W
        assert f.opts.solve_waves == W and f1.opts.solve_waves == 1
        x, y, st, qs = _solve(f, warm_start=0)
        prev = (x, y)
        for variant in QP_VARIANTS:
            opts = VARIANTS[variant]
            x, y, st, qs = _solve(f, warm_start=0, **opts)
            solved = _check(f"{model} waves={W}", qps, refs, lps, x, y, st, prev, variant, opts.get("qp_eps", 1e-6))
            prev = (x, y)
            assert solved, variant
            assert np.array_equal(qs[:, 6], st), variant
            st1 = _solve(f1, warm_start=0, **opts)[2]
            keep = _must_match(P)
            assert np.array_equal(st[keep], st1[keep]), (variant, [(qps[b].name, st[b], st1[b]) for b in keep if st[b] != st1[b]])
            if variant == "max_iter8":
                assert (st == 1).any(), variant
        assert f.factor_stages > 0 and f.factor_stages % qps[0].N == 0      # (whole factorisations only)
    finally:
        f.close(); f1.close()


@pytest.mark.parametrize("W", [2, 8])
@pytest.mark.parametrize("model", QC.PLANTS)
def test_qp_paths_warm_multiwave(model, W):
    """Solve, move q and the bounds a little, solve again warm (as tests/test_gpu_qp_paths.py::test_qp_paths_warm) -- the warm solve under every variant:
    as_max_viol0 abandons the warm attempt at once and factorises afresh in the interior point after solve-only ticks, max_iter8 ends some QPs with
    status 1 and the first solve's x / y kept, as_first0 goes to the interior point directly.  A handle with one wave goes through the same sequence:
    the statuses of the moved QPs (all clearly feasible: LP margin <= -1e-3) must be the same."""
    P = _plant(model)
    refs, lps = P["refs"], P["lps"]
    base, moved, mrefs, mlps = _moved(model)
    keep = [P["qps"].index(q) for q in base]
    must = [b for b, q in enumerate(moved) if q.cls == "x0edge" or mlps[b][0] <= -1e-3]
    assert must
    f, f1 = make_gpu_solver_qp(base), make_gpu_solver_qp(base)
    try:
        f.opts.solve_waves = W
        for variant in QP_VARIANTS:
            opts = VARIANTS[variant]
            second = {}
            for g in (f, f1):
                _push(g, base)
                x1, y1, st1, _ = _solve(g, warm_start=0)
                if g is f:
                    _check(f"{model} waves={W}", base, [refs[b] for b in keep], [lps[b] for b in keep], x1, y1, st1, (x1, y1), "warm-first")
                _push(g, moved)
                second[g is f] = (x1, y1, st1) + _solve(g, warm_start=1, **opts)
            x1, y1, st1, x2, y2, st2, qs2 = second[True]
            solved = _check(f"{model} waves={W}", moved, mrefs, mlps, x2, y2, st2, (x1, y1), f"warm-second {variant}", opts.get("qp_eps", 1e-6))
            assert solved, variant
            assert np.array_equal(qs2[:, 6], st2), variant
            if variant == "default":
                for b in range(len(base)):
                    if st1[b] == 0:
                        assert qs2[b, 4] == 1, (model, moved[b].name, qs2[b])            # warm source 1: the previous call's set
                assert (qs2[:, 4] == 1).any()
            st2_1 = second[False][5]
            assert np.array_equal(st2[must], st2_1[must]), (variant, [(moved[b].name, st2[b], st2_1[b]) for b in must if st2[b] != st2_1[b]])
    finally:
        f.close(); f1.close()


@functools.lru_cache(maxsize=None)
def _moved(model):
    P = _plant(model)
    qps, lps = P["qps"], P["lps"]
    keep = [b for b, q in enumerate(qps) if lps[b][1] == "feasible" and lps[b][0] <= -1e-3 and q.cls in ("easy", "stress", "bigset", "scaled")]
    base = [qps[b] for b in keep]
    rng = np.random.default_rng(7)
    moved = []
    for q in base:
        c = q.copy(name=q.name + "-moved")
        c.q = q.q * (1.0 + 1e-3 * rng.uniform(-1, 1, q.q.size))
        hi, lo = q.boxes()
        for e in range(q.nx, q.n):
            if abs(hi[e]) < QC.BIG:
                c.set_box(e, hi=hi[e] + 1e-4 * rng.uniform(-1, 1))
            if abs(lo[e]) < QC.BIG:
                c.set_box(e, lo=lo[e] + 1e-4 * rng.uniform(-1, 1))
        moved.append(c)
    return base, moved, [QC.reference(q) for q in moved], [QC.feasibility_margin(q) for q in moved]


@pytest.mark.parametrize("model", QC.PLANTS)
def test_switching_paths_on_one_handle(model):
    """1 wave after 8 and the reverse on the same handle, warm: the same host checks (neither path reads the other's stored factors), and a handle
    whose option was never touched gives the bits of another untouched one."""
    P = _plant(model)
    qps, refs, lps = P["qps"], P["refs"], P["lps"]
    base, moved, mrefs, mlps = _moved(model)
    keep = [qps.index(q) for q in base]
    f, g0, g1 = make_gpu_solver_qp(base), make_gpu_solver_qp(base), make_gpu_solver_qp(base)
    try:
        xa, ya, sta, _ = _solve(g0, warm_start=0)
        xb, yb, stb, _ = _solve(g1, warm_start=0)
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb) and np.array_equal(sta, stb)
        prev = None
        for i, W in enumerate((8, 1, 8, 1)):
            f.opts.solve_waves = W
            cur, crefs, clps = (base, [refs[b] for b in keep], [lps[b] for b in keep]) if i % 2 == 0 else (moved, mrefs, mlps)
            _push(f, cur)
            x, y, st, qs = _solve(f, warm_start=1 if i else 0)
            _check(f"{model} switch {i} waves={W}", cur, crefs, clps, x, y, st, prev or (x, y), "default")
            prev = (x, y)
    finally:
        f.close(); g0.close(); g1.close()


# ---- 3. fast-SLS and closed loop --------------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("model", QC.PLANTS)
def test_fast_sls_step_agrees_with_one_wave(model, steps, B):
    insts = [make_instance(model, s, 0.5) for s in range(B)]
    outs = {}
    for W in (1, 4):
        f = make_gpu_solver(insts)
        try:
            f.opts.solve_waves = W
            outs[W] = run_gpu_fastsls(insts, rti_steps=steps, solver=f)
        finally:
            f.close()
    o, r = outs[4], outs[1]
    assert r["success"].all()
    for k in ("status", "success", "iteration_number"):
        assert np.array_equal(o[k], r[k]), (k, o[k], r[k])
    for k in ("primal_vec", "backoff_x", "backoff_u", "eta"):
        assert _rel(o[k], r[k]) < 1e-6, (k, _rel(o[k], r[k]))


@pytest.mark.parametrize("model,N,steps", [("pendulum", 10, 10), ("rocket", 20, 3)])
def test_closed_loop_agrees_with_one_wave(model, N, steps):
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, disturbance_stream, get_model
    m = get_model(model)
    if model == "pendulum":
        x0, W, kw = m.extra["x0"][None], None, dict(solve_nominal=True)
    else:
        x0, W, kw = (m.x_ref + 0.01 * (m.extra["x0"] - m.x_ref))[None], disturbance_stream(0, steps, m.nx)[:, None], dict(solve_nominal=True, continuation=2)
    outs = {}
    for waves in (1, 4):
        cl = ClosedLoopMPC(m, N, 1, solve_waves=waves)
        try:
            assert cl.f.opts.solve_waves == waves
            outs[waves] = cl.run_on_device(x0, steps, W, **kw)
        finally:
            cl.close()
    o, r = outs[4], outs[1]
    assert r["success"].all() and np.array_equal(o["success"], r["success"])
    for k in ("state_trajectory", "input_trajectory"):
        assert _rel(o[k], r[k]) < 1e-6, (k, _rel(o[k], r[k]))


def test_refusals_and_fallback():
    import ctypes as C
    from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model
    m = get_model("pendulum")
    x0 = np.tile(m.extra["x0"], (2, 1))
    cl = ClosedLoopMPC(m, 10, 2, solve_waves=2)
    try:
        f, lib = cl.f, cl.f.lib
        for bad in (3, 0, 16, -2):
            with pytest.raises(RuntimeError, match="1 .*2, 4 or 8"):
                f.opts.solve_waves = bad
            assert f.opts.solve_waves == 2
        cl.reset(x0)
        rounds = C.c_int(0)
        assert lib.slsqp_cl_run_scp(f.h, 2, cl.rti, None, 0, C.byref(f.opts)) < 0 and b"solve_waves" in lib.slsqp_last_error()
        o1 = type(f.opts)()
        C.memmove(C.byref(o1), C.byref(f.opts), C.sizeof(o1))
        o1.rti_steps = 1
        assert lib.slsqp_cl_run(f.h, 2, None, 0, C.byref(o1), 8.0, 0.0, C.byref(rounds)) < 0 and b"solve_waves" in lib.slsqp_last_error()
        f.opts.precision = 1
        with pytest.raises(RuntimeError, match="fp64 only"):
            cl.step()
        f.opts.precision = 0
        out = cl.run_decoupled(x0, 3)                       # falls back to the step-by-step loop
        assert out["success"].shape == (2, 3) and "loop_stats" not in out
        ref = ClosedLoopMPC(m, 10, 2)
        try:
            r = ref.run_on_device(x0, 3)
        finally:
            ref.close()
        assert np.array_equal(out["success"], r["success"]) and _rel(out["state_trajectory"], r["state_trajectory"]) < 1e-6
    finally:
        cl.close()


def test_new_entry_points_under_debug_allocators():
    """slsqp_ne_solve and the solve_waves setter / getter in a child process whose allocators check their block boundaries (as
    tests/test_gpu_parity.py::test_python_mirror_under_debug_allocators for the entry points that were there before)."""
    import subprocess
    env = dict(os.environ, MALLOC_CHECK_="3", PYTHONMALLOC="malloc_debug")
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.join(ROOT, "tests", "abi_memcheck_multiwave.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "abi_memcheck_multiwave ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

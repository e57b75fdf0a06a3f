"""The single-wave sweeps at the horizons where a moved or clamped stage load can go wrong: N = 1, 2, 3 (4 for the block solve).

The forward sweep prefetches stage k + 1 while it works on stage k and the backward sweep keeps two stages in flight in two register sets, the
last two reloads of which read stage 0 again.  With N = 1 there is no prefetch at all, with N = 2 every reload of the backward
sweep is a clamped one, N = 3 has the odd tail stage, N = 4 is the first horizon whose backward loop runs twice.  Plants: pendulum (4, 1: the
vector-ALU path), quadrotor (13, 4) and rocket (17, 4), three instances each.

1. slsqp_ne_solve with one wave: a factorisation and then a substitution-only call (eflag = 0, factorising and solve-only stages) against the
   host system of tests/test_gpu_multiwave.py's helpers.  G against E' nu to that file's 1e-12.  The residual against the host prototype's
   (scripts/proto/cr_normal_eq.py, the same block elimination in numpy): the library of the commit before the prefetch change gives a worst
   ratio of 11.37 on exactly these inputs (MI355X: pendulum, N = 1, late-ipm weighting, the factorising call, instance 2, where the
   prototype's own residual is 3e-17; per plant and horizon the worst ratios lie between 1.5 and 11.4); the cap is twice that, rounded up to
   one digit, 30 -- the code is meant to be bit-equal to that library, the factor covers last-bit differences between runs only.
2. slsqp_qp_solve cold and then warm against the dense interior point of tests/ref_ipm.py, with the assertions and tolerances of
   tests/test_gpu_qp_paths.py::_check for the default options (primal to 1e-6, host certificate, verdicts supported by the phase-1 LP,
   feasible with margin means solved).  Between the two solves the last stage's input boxes are widened, so the warm attempt from the
   previous set needs a further active-set round whose set differs from stage N - 1 on only: an eflag = 1 sweep with ks = N - 1.  The
   library records no ks; the test asserts the warm source and that such a round ran.
3. The persistent launch (k_cl_loop: all four sweeps inlined) against slsqp_cl_step, three MPC steps: the same bits.  No existing test runs
   a closed loop below N = 10.
"""
import functools

import numpy as np
import pytest

import qp_corpus as QC
from problems import make_instance, qp1_bounds
from test_gpu_multiwave import CR, DELTA, _la_solver, _la_systems
from test_gpu_qp_paths import _check, _push, _solve, make_gpu_solver_qp
from test_gpu_reference import _assert_same, _decoupled, _make, _seeded_W, _stepwise

pytestmark = pytest.mark.gpu

PARENT_WORST_RATIO = 11.37    # measured with the parent commit's library, see the module docstring
RATIO_CAP = 30.0              # 2 x PARENT_WORST_RATIO = 22.7, rounded up to one digit


def _block_solve_ratios(model, N):
    """[(what, device residual / prototype residual)] of the factorisation and the substitution-only call, both weightings, three instances;
    finiteness, the failure flags and G = E' nu are asserted on the way."""
    ratios = []
    for weighting in ("active-set", "late-ipm"):
        A, B, PI, m = _la_systems(model, N, weighting)
        Bn, n = A.shape[0], PI.shape[1]
        assert Bn == 3
        rng = np.random.default_rng(100 + N)
        rhs = (rng.normal(size=(Bn, n)), rng.normal(size=(Bn, n)))
        sysm = [CR.stage_blocks(A[b], B[b], PI[b], DELTA) for b in range(Bn)]
        f = _la_solver(m, N, A, B)
        try:
            outs = [f.ne_solve(PI, rhs[0], waves=1, factor=True, delta=DELTA), f.ne_solve(PI, rhs[1], waves=1, factor=False, delta=DELTA)]
        finally:
            f.close()
        for which, (out, V) in enumerate(zip(outs, rhs)):
            tag = f"{model} N={N} {weighting} {'factorisation' if which == 0 else 'substitution only'}"
            assert np.isfinite(out["nu"]).all() and np.isfinite(out["G"]).all() and (out["fail"] == 0).all(), tag
            for b in range(Bn):
                bh = CR.rhs(A[b], B[b], V[b])
                D, O = sysm[b]
                r = CR.residual(D, O, bh, out["nu"][b])
                proto = CR.residual(D, O, bh, CR.cr(D, O, bh)[0])
                print(f"{tag} instance {b}: residual {r:.2e}, prototype {proto:.2e}, ratio {r / proto:.3f}")
                ratios.append((f"{tag} instance {b}", float(r / proto)))
                G = CR.E_t_nu(A[b], B[b], out["nu"][b])
                assert np.abs(out["G"][b] - G).max() <= 1e-12 * max(np.abs(G).max(), 1e-300), tag
    return ratios


@pytest.mark.parametrize("N", [1, 2, 3, 4])
@pytest.mark.parametrize("model", QC.PLANTS)
def test_single_wave_block_solve_at_short_horizons(model, N):
    ratios = _block_solve_ratios(model, N)
    what, worst = max(ratios, key=lambda t: t[1])
    print(f"{model} N={N}: worst residual ratio against the prototype {worst:.3f} ({what})")
    assert worst <= RATIO_CAP, (what, worst)


@functools.lru_cache(maxsize=None)
def _short_qps(model, N):
    """three QPs of the plant at horizon N (an easy one and two with x_0 far out and the input boxes at 8 % of their width, so that bounds are
    active and the active-set rounds have something to do), their moved twins for the warm solve, and the references and LP verdicts of both --
    computed once per (model, N)"""
    base = []
    for seed, amp in ((0, 0.5), (1, 2.0), (2, 2.0)):
        inst = make_instance(model, seed, amp, N=N)
        l, u = qp1_bounds(inst)
        qp = QC.QP(inst.m, N, inst.A, inst.B, inst.q, l, u, "easy" if amp < 1.0 else "bigset", f"N{N}-{seed}")
        if amp > 1.0:
            hi, lo = qp.boxes()
            for k in range(N):
                for e in range(k * qp.nz + qp.nx, (k + 1) * qp.nz):
                    if 0.0 < hi[e] < QC.BIG:
                        qp.set_box(e, hi=0.08 * hi[e])
                    if -QC.BIG < lo[e] < 0.0:
                        qp.set_box(e, lo=0.08 * lo[e])
        base.append(qp)
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
        if q.cls == "bigset":
            # the last stage's input boxes go back to their full width: bounds that were active there let go, so the warm attempt from the
            # previous set needs another active-set round, and that round's set differs from the one before from stage N - 1 on only
            # (the forward sweep's k0 = ks = N - 1 > 0 for N >= 2)
            for e in range((N - 1) * q.nz + q.nx, N * q.nz):
                if 0.0 < hi[e] < QC.BIG:
                    c.set_box(e, hi=hi[e] / 0.08)
                if -QC.BIG < lo[e] < 0.0:
                    c.set_box(e, lo=lo[e] / 0.08)
        moved.append(c)
    ref = lambda qs: ([QC.reference(q) for q in qs], [QC.feasibility_margin(q) for q in qs])      # noqa: E731
    return base, moved, ref(base), ref(moved)


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("model", QC.PLANTS)
def test_cold_then_warm_qp_solve_at_short_horizons(model, N):
    base, moved, (refs, lps), (mrefs, mlps) = _short_qps(model, N)
    f = make_gpu_solver_qp(base)
    try:
        x1, y1, st1, qs1 = _solve(f, warm_start=0)
        solved = _check(f"{model} N={N} cold", base, refs, lps, x1, y1, st1, (x1, y1), "default")
        assert solved, (model, N, st1)
        _push(f, moved)
        x2, y2, st2, qs2 = _solve(f, warm_start=1)
        solved2 = _check(f"{model} N={N} warm", moved, mrefs, mlps, x2, y2, st2, (x1, y1), "default")
        assert solved2, (model, N, st2)
        print(f"{model} N={N}: cold status {st1}, qp_stats {qs1.tolist()}; warm status {st2}, qp_stats {qs2.tolist()}")
        for b in solved:
            if st1[b] == 0:
                assert qs2[b, 4] == 1, (model, N, moved[b].name, qs2[b])            # warm source 1: the previous call's set
        # the library has no counter for ks; what it records is the warm source and the active-set rounds.  A warm solve that needed a round
        # beyond its first attempt changed its set where the boxes were moved, at stage N - 1, so that round's forward sweep ran eflag = 1
        # with k0 = ks = N - 1 (> 0 for N >= 2)
        assert any(qs2[b, 4] == 1 and qs2[b, 5] >= 1 for b in solved2), (model, N, qs2.tolist())
    finally:
        f.close()


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("model", QC.PLANTS)
def test_persistent_launch_is_the_step_by_step_loop_at_short_horizons(model, N):
    from robust_nonlinear_mpc_amd import get_model
    m = get_model(model)
    B, steps = 3, 3
    far = m.extra["x0"] if "x0" in m.extra else m.x_ref + 0.05 * (m.x_ub - m.x_lb)
    x0 = np.stack([m.x_ref + s * (far - m.x_ref) for s in (0.1, 0.2, 0.3)])
    W = _seeded_W(m, B, steps)
    ref, ref_fin = _stepwise(_make(m, N, B, 1, 1), steps, x0, W)
    print(f"{model} N={N}: success rate {ref['success'].mean():.2f}")
    assert np.isfinite(ref["state_trajectory"]).all()
    out, fin = _decoupled(_make(m, N, B, 1, 1), steps, x0, W)
    _assert_same(out, fin, ref, ref_fin, f"{model} N={N} persistent")

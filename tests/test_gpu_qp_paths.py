"""Every QP solve path and every verdict against the independent host checks of tests/qp_corpus.py.

The QP is strictly convex, so every option variant must reach the reference optimum (tests/ref_ipm.py) or give a verdict the phase-1 LP
supports.  Per instance and variant:
  - the status is one of 0-5 (never -1: ST_INIT left behind);
  - status 0 / 4: finite outputs, host certificate, primal to 1e-6 of the reference (multipliers too where strictly complementary);
  - status 2 exactly when x_0 is more than 1e-9 outside its stage-0 box; 2 / 5 only where the LP says infeasible or borderline;
  - any status but 0 / 4 leaves that instance's x and y as the call before left them, bit for bit;
  - each variant's qp_stats show that the path it exists for ran.
Non-finite data in one instance of a batch ends that instance unsolved and leaves the others bitwise untouched.
"""
import numpy as np
import pytest

import qp_corpus as QC
from problems import make_instance, make_gpu_solver, push_instances, qp1_bounds, run_gpu_fastsls, stack

pytestmark = pytest.mark.gpu

VARIANTS = {
    "default": {},
    "as_first0": dict(as_first=0),
    "as_first1": dict(as_first=1),
    "as_max_viol0": dict(as_max_viol=0),
    "as_rounds1": dict(as_rounds=1),
    "qp_eps1e-3": dict(qp_eps=1e-3, as_first=0),
    "precision1": dict(precision=1),
    "max_iter8": dict(qp_max_iter=8, as_first=0),
}


@pytest.fixture(scope="module", params=QC.PLANTS)
def plant(request):
    qps = QC.corpus(request.param)
    return dict(model=request.param, qps=qps, refs=[QC.reference(q) for q in qps], lps=[QC.feasibility_margin(q) for q in qps])


def _push(f, qps, A=None, Bm=None):
    m, N, B = qps[0].m, qps[0].N, len(qps)
    f.update_dynamics_list(stack(qps, "A") if A is None else A, stack(qps, "B") if Bm is None else Bm, np.stack([m.E] * (N + 1)),
                           np.zeros((B, N, m.ni)), np.zeros((B, m.ni_f)), np.zeros((B, N, m.nx)))
    f.qp_update_data_vec(stack(qps, "q"), stack(qps, "l"), stack(qps, "u"))


def _solve(f, **opts):
    saved = {k: getattr(f.opts, k) for k in opts}
    for k, v in opts.items():
        setattr(f.opts, k, v)
    try:
        f.kernel_timing()                       # (resets the accumulators)
        x, y, st, it, _ = f.qp_solve()
        f.kernel_timing()
        qs = f.get("qp_stats", (2, 8), np.int32)[:, 0]
    finally:
        for k, v in saved.items():
            setattr(f.opts, k, v)
    return x, y, st, qs


def _check(P, qps, refs, lps, x, y, st, prev, variant, qp_eps=1e-6):
    """The per-instance assertions of the module docstring; returns the instance indices that ended 0 / 4."""
    solved = []
    for b, qp in enumerate(qps):
        tag = f"{P} {variant} {qp.name}: status {st[b]}"
        assert st[b] in (0, 1, 2, 3, 4, 5), tag
        assert (st[b] == 2) == (qp.x0_violation() > 1e-9), tag
        t, verdict = lps[b]
        if st[b] in (2, 5):
            assert verdict in ("infeasible", "borderline"), f"{tag}, LP t* = {t:.3e}"
        if st[b] in (0, 4):
            solved.append(b)
            ok, rep = QC.host_certificate(qp, x[b], y[b], st[b], qp_eps)
            assert ok, f"{tag}: certificate {rep}"
            ref = refs[b]
            assert ref is not None, f"{tag}: solved, but the reference finds no optimum (LP t* = {t:.3e})"
            # (the certificate is relative to max(1, |q|inf): with q scaled by 1e4 it admits 1e4 times the absolute residual, and bounds whose
            # multipliers lie below that may be taken as active by one solver and not by the other)
            err = QC.relerr(x[b], ref["x"])
            assert err < (1e-5 if st[b] == 4 or qp.cls == "scaled" else 1e-6), f"{tag}: primal off by {err:.2e}"
            if st[b] == 0 and ref["strict"] and qp.cls != "scaled":
                sc = qp.qscale()
                assert np.max(np.abs(y[b] - ref["y"])) < 1e-6 * max(sc, np.abs(ref["y"]).max()), f"{tag}: multipliers"
        else:
            assert np.array_equal(x[b], prev[0][b]) and np.array_equal(y[b], prev[1][b], equal_nan=True), f"{tag}: previous x / y not kept"
        if variant == "default" and verdict == "feasible" and t <= -1e-3:
            assert st[b] in (0, 4), f"{tag}: feasible with margin {t:.3e} but not solved"
    names = {q.name: b for b, q in enumerate(qps)}
    for b, qp in enumerate(qps):           # +-1e20 and +-inf: no bound either way, the same answer bit for bit
        if qp.twin is not None:
            o = names[qp.twin]
            assert st[b] == st[o] and np.array_equal(x[b], x[o]), (variant, qp.name)
    return solved


def test_qp_paths_cold(plant):
    P, qps, refs, lps = plant["model"], plant["qps"], plant["refs"], plant["lps"]
    f = make_gpu_solver_qp(qps)
    try:
        x, y, st, qs = _solve(f, warm_start=0)
        prev = (x, y)
        its = {}
        for variant, opts in VARIANTS.items():
            x, y, st, qs = _solve(f, warm_start=0, **opts)
            its[variant] = qs[:, 0].copy()
            solved = _check(P, qps, refs, lps, x, y, st, prev, variant, opts.get("qp_eps", 1e-6))
            prev = (x, y)
            assert solved, variant
            it, path = qs[:, 0], qs[:, 7]
            if "precision" not in opts:
                assert np.array_equal(qs[:, 6], st), variant           # qp_stats record the same status
            if variant in ("default", "as_first1"):
                assert any(it[b] == 0 and st[b] == 0 for b in solved), variant      # the active-set attempt from the empty set certified
            if variant in ("as_first0", "qp_eps1e-3"):
                # every solved instance went through the interior point (a QP without any finite bound is solved by its starting point)
                assert all(it[b] > 0 for b in solved if np.abs(np.concatenate(qps[b].boxes())).min() < QC.BIG), variant
            if variant in ("as_max_viol0", "as_rounds1"):
                assert any(path[b] == 1 for b in solved), variant                   # abandoned active-set attempt, then the interior point
            if variant == "qp_eps1e-3":
                # the loose interior point's polish was rejected somewhere: status 4, or the resume towards 1e-9 (more iterations than a 1e-6 run)
                assert (st == 4).any() or any(its[variant][b] > its["as_first0"][b] for b in solved), variant
            if variant == "precision1":
                assert f.mx_retries > 0 or all(s_ in (0, 2, 5) for s_ in st), variant      # the fp64 re-solve ran wherever it had to
            if variant == "max_iter8":
                assert (st == 1).any(), variant
    finally:
        f.close()


def make_gpu_solver_qp(qps):
    from robust_nonlinear_mpc_amd import BatchedFastSLS
    m, N = qps[0].m, qps[0].N
    f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=len(qps))
    _push(f, qps)
    return f


@pytest.mark.parametrize("warm_rounds", [None, 1])
def test_qp_paths_warm(plant, warm_rounds):
    """Solve, move q and the bounds a little, solve again warm: the same checks, and the second solve starts from the first one's set."""
    P, qps, refs, lps = plant["model"], plant["qps"], plant["refs"], plant["lps"]
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
    mrefs, mlps = [QC.reference(q) for q in moved], [QC.feasibility_margin(q) for q in moved]
    f = make_gpu_solver_qp(base)
    opts = {} if warm_rounds is None else dict(warm_rounds=warm_rounds)
    try:
        x1, y1, st1, _ = _solve(f, warm_start=0, **opts)
        _check(P, base, [refs[b] for b in keep], [lps[b] for b in keep], x1, y1, st1, (x1, y1), "warm-first")
        _push(f, moved)
        x2, y2, st2, qs2 = _solve(f, warm_start=1, **opts)
        _check(P, moved, mrefs, mlps, x2, y2, st2, (x1, y1), f"warm-second (warm_rounds {warm_rounds})")
        for b in range(len(base)):
            if st1[b] == 0:
                assert qs2[b, 4] == 1, (P, moved[b].name, qs2[b])            # warm source 1: the previous call's set
        assert (qs2[:, 4] == 1).any()
    finally:
        f.close()


# ---- non-finite data in one instance ---------------------------------------------------------------------------
BAD = 3


def _poisons(nx, nz, N, SR):
    """(field, index, value): q, one upper-bound row, one lower-bound row, c, A, B, x0 -- NaN each, and +-inf but for the bounds."""
    e = (N // 2) * nz + nx + 1            # an element of a middle stage
    k = N // 2
    out = []
    for v in (np.nan, np.inf, -np.inf):
        out += [("q", e, v), ("c", (k, 1), v), ("A", (k, 1, 2), v), ("B", (k, 1, 0), v), ("x0", 1, v)]
    out += [("hi", e, np.nan), ("lo", e, np.nan)]
    return out


@pytest.mark.parametrize("precision", [0, 1])
def test_non_finite_data_qp_level(precision):
    insts = [make_instance("rocket", s, 0.5) for s in range(8)]
    m, N = insts[0].m, insts[0].N
    nx, nz, SR = m.nx, m.nz, m.nx + m.ni
    lu = [qp1_bounds(i) for i in insts]
    qps = [QC.QP(m, N, i.A, i.B, i.q, l, u, "easy", f"easy-{b}") for b, (i, (l, u)) in enumerate(zip(insts, lu))]
    f = make_gpu_solver_qp(qps)
    try:
        clean = _solve(f, warm_start=0, precision=precision)
        assert (clean[2] == 0).all()
        for field, idx, v in _poisons(nx, nz, N, SR):
            q, l, u = stack(qps, "q"), stack(qps, "l"), stack(qps, "u")
            A, Bm = stack(qps, "A"), stack(qps, "B")
            if field == "q":
                q[BAD, idx] = v
            elif field == "hi":
                u[BAD, qps[0].hi_row(idx)] = v
            elif field == "lo":
                u[BAD, qps[0].lo_row(idx)] = v
            elif field == "c":
                r = idx[0] * SR + idx[1]
                l[BAD, r] = u[BAD, r] = v
            elif field == "A":
                A[(BAD,) + idx] = v
            elif field == "B":
                Bm[(BAD,) + idx] = v
            elif field == "x0":
                l[BAD, qps[0].mb + idx] = u[BAD, qps[0].mb + idx] = v
            _push(f, qps, A, Bm)
            f.qp_update_data_vec(q, l, u)
            x, y, st, qs = _solve(f, warm_start=0, precision=precision)
            tag = f"{field} = {v}: status {st[BAD]}"
            # x0 NaN / inf: outside every box, status 2; non-finite q, bound rows, c, A, B: flagged around the launch, status 3
            assert st[BAD] == (2 if field == "x0" else 3), tag
            assert qs[BAD, 6] == st[BAD], tag
            # flagged without taking part in the launch: the answer of the last solve that certified stays, bit for bit
            assert np.array_equal(x[BAD], clean[0][BAD]) and np.array_equal(y[BAD], clean[1][BAD]), tag
            ok = [b for b in range(8) if b != BAD]
            assert np.array_equal(st[ok], clean[2][ok]) and np.array_equal(x[ok], clean[0][ok]) and np.array_equal(y[ok], clean[1][ok]), tag
            _push(f, qps)
        # an upper bound of +inf is no bound, exactly like +1e20
        outs = []
        for v in (1e20, np.inf):
            u = stack(qps, "u")
            u[BAD, qps[0].hi_row(4 * nz + nx)] = v
            f.qp_update_data_vec(stack(qps, "q"), stack(qps, "l"), u)
            outs.append(_solve(f, warm_start=0, precision=precision))
        for a, b in zip(outs[0][:3], outs[1][:3]):
            assert np.array_equal(a, b)
    finally:
        f.close()


def _fast_sls(insts, route):
    """one RTI fast-SLS step on a fresh handle (no state carried over from another batch)"""
    f = make_gpu_solver(insts)
    for k, v in route.items():
        setattr(f.opts, k, v)
    try:
        return run_gpu_fastsls(insts, rti_steps=1, solver=f)
    finally:
        f.close()


@pytest.mark.parametrize("route", [dict(fuse_rti=0), dict(fuse_rti=2), dict(precision=1, fuse_rti=0)], ids=["separate", "fused", "mixed"])
def test_non_finite_data_fast_sls(route):
    insts = [make_instance("rocket", s, 0.5) for s in range(8)]
    m, N = insts[0].m, insts[0].N
    nx, nz = m.nx, m.nz
    clean = _fast_sls(insts, route)
    assert clean["success"].all()
    k0 = N // 2
    cases = []
    for v in (np.nan, np.inf, -np.inf):
        cases += [("q", v), ("c", v), ("A", v), ("B", v), ("x0", v)]
    cases += [("g_hi", np.nan), ("g_lo", np.nan)]
    for field, v in cases:
        bad = [make_instance("rocket", s, 0.5) for s in range(8)]
        i = bad[BAD]
        if field == "q":
            i.q = i.q.copy(); i.q[k0 * nz + nx + 1] = v
        elif field == "c":
            i.c = i.c.copy(); i.c[k0, 1] = v
        elif field == "A":
            i.A = i.A.copy(); i.A[k0, 1, 2] = v
        elif field == "B":
            i.B = i.B.copy(); i.B[k0, 1, 0] = v
        elif field == "x0":
            i.x0_arg = i.x0_arg.copy(); i.x0_arg[1] = v
        elif field == "g_hi":
            i.g_list = list(i.g_list); i.g_list[k0] = i.g_list[k0].copy(); i.g_list[k0][nx + 1] = v
        elif field == "g_lo":
            i.g_list = list(i.g_list); i.g_list[k0] = i.g_list[k0].copy(); i.g_list[k0][nz + nx + 1] = v
        out = _fast_sls(bad, route)
        tag = f"{route} {field} = {v}: status {out['status'][BAD]}"
        assert not out["success"][BAD] and out["status"][BAD] == (2 if field == "x0" else 3), tag
        ok = [b for b in range(8) if b != BAD]
        for key in ("success", "status", "primal_vec", "backoff", "dual_vec"):
            assert np.array_equal(out[key][ok], clean[key][ok]), (tag, key)


# ---- fast-SLS level: the options of the call's second QP and of consecutive calls ------------------------------------
FAST_VARIANTS = {
    "as_warm_max_set0": dict(as_warm_max_set=0), "as_warm_max_set1": dict(as_warm_max_set=1),
    "as_warm_last0": dict(as_warm_last=0), "as_warm_last2": dict(as_warm_last=2),
    "ipm_restart0": dict(ipm_restart=0), "as_first0": dict(as_first=0), "as_first1": dict(as_first=1),
    "precision1": dict(precision=1), "fuse_rti0": dict(fuse_rti=0), "fuse_rti2": dict(fuse_rti=2),
}


def _fast_insts(model):
    """stress instances (x0 amplitude 2, Jacobian noise 1e-2, defects 1e-2) and big-set ones (input boxes at 8 % of their width)"""
    out = []
    for s in range(4):
        i = make_instance(model, 100 + s, 2.0, c_amp=1e-2)
        rng = np.random.default_rng(900 + s)
        i.A = i.A + 1e-2 * rng.normal(size=i.A.shape); i.B = i.B + 1e-2 * rng.normal(size=i.B.shape)
        out.append(i)
    for s in range(4):
        i = make_instance(model, 110 + s, 0.6)
        nx, nz = i.m.nx, i.m.nz
        g = [np.array(x, dtype=float) for x in i.g_list]
        for k in range(i.N):
            for j in (np.arange(nx, nz), np.arange(nz + nx, 2 * nz)):
                g[k][j] = np.where(g[k][j] > 0, 0.08 * g[k][j], g[k][j])
        i.g_list = g
        out.append(i)
    return out


def _fast_run(insts, opts, rti):
    """two calls on one handle (the second with a moved measured state), qp_stats of both"""
    f = make_gpu_solver(insts)
    for k, v in opts.items():
        setattr(f.opts, k, v)
    try:
        outs, qss = [], []
        for call in range(2):
            x0 = stack(insts, "x0_arg") * (1.0 + 0.05 * call)
            f.set_rti_steps(rti)
            push_instances(f, insts)
            outs.append(f.solve(x0))
            qss.append(f.get("qp_stats", (2, 8), np.int32))
        return outs, qss
    finally:
        f.close()


@pytest.mark.parametrize("model,rti", [("rocket", 1), ("quadrotor", 2)])
def test_fast_sls_option_variants_agree(model, rti):
    """Every option that picks a different warm start or restart of the call's QPs reaches the same answers as the defaults: primal and back-offs
    to 1e-6, the same success flags; and the paths the options exist for ran."""
    insts = _fast_insts(model)
    ref, ref_qs = _fast_run(insts, {}, rti)
    assert ref[1]["success"].any()
    seen = {}
    for name, opts in FAST_VARIANTS.items():
        outs, qss = _fast_run(insts, opts, rti)
        for call in range(2):
            o, r = outs[call], ref[call]
            assert np.array_equal(o["success"], r["success"]), (name, call, o["status"], r["status"])
            for b in np.flatnonzero(r["success"]):
                assert QC.relerr(o["primal_vec"][b], r["primal_vec"][b]) < 1e-6, (name, call, b)
                assert QC.relerr(o["backoff"][b], r["backoff"][b]) < 1e-6, (name, call, b)
        seen[name] = qss[1]
    # warm source of the second call's last QP: 2 (the previous call's last set) under as_warm_last = 2, never under 0
    assert (seen["as_warm_last2"][:, 1, 4] == 2).any()
    assert not (seen["as_warm_last0"][:, 1, 4] == 2).any()
    # as_warm_max_set = 1: the last QP no longer starts from the first QP's set (source 1) where that set has more than one active bound
    src_ref, src1 = ref_qs[1][:, 1, 4], seen["as_warm_max_set1"][:, 1, 4]
    assert (src1 == 1).sum() <= (src_ref == 1).sum()
    if (src_ref == 1).any():
        assert ((src_ref == 1) & (src1 != 1)).any()

"""The corpus of tests/qp_corpus.py and its host checks, tested without a GPU: every class is what it claims to be, the two exact
references agree, and the host certificate passes the reference optimum and fails it once it is disturbed."""
import numpy as np
import pytest

import qp_corpus as QC


@pytest.fixture(scope="module", params=QC.PLANTS)
def plant(request):
    qps = QC.corpus(request.param)
    return dict(model=request.param, qps=qps, refs=[QC.reference(q) for q in qps], lps=[QC.feasibility_margin(q) for q in qps])


def test_classes_are_what_they_claim(plant):
    P, qps, refs, lps = plant["model"], plant["qps"], plant["refs"], plant["lps"]
    names = [q.name for q in qps]
    assert len(set(names)) == len(names)
    assert {q.cls for q in qps} == {"easy", "stress", "bigset", "degenerate", "x0edge", "infeasible", "scaled"}
    for q, ref, (t, verdict) in zip(qps, refs, lps):
        tag = f"{P} {q.name}: LP t* = {t:.3e} ({verdict})"
        if q.intent == "feasible":
            assert verdict in ("feasible", "borderline"), tag
        if q.intent == "infeasible":
            assert verdict == "infeasible" and q.x0_violation() <= 0.0, tag       # x0 inside its box, infeasible further down the horizon
        if q.cls in ("easy", "bigset", "scaled") or q.name.startswith("nobox"):
            assert verdict == "feasible" and t <= -1e-3, tag
        if verdict == "infeasible":
            assert ref is None or q.x0_violation() <= 1e-9, tag
        if verdict != "infeasible" and q.x0_violation() <= 1e-9:
            assert ref is not None and ref["kkt"] < 1e-9, tag           # the reference optimum exists and is certified by its own residual
    x0 = {q.name.split("-")[1]: q.x0_violation() for q in qps if q.cls == "x0edge"}
    assert x0["0"] <= 0.0 and 0.0 < x0["5e"] < 1e-9 and 1e-9 < x0["1e"] and x0["1"] > 0.5
    # borderline band: only the instances built on an edge land in it
    for q, (t, verdict) in zip(qps, lps):
        if verdict == "borderline":
            assert q.cls in ("x0edge", "degenerate"), (P, q.name, t)
    # the big-set class: a quarter or more of its instances with >= 29 active bounds (the plants with room for them)
    big = [ref["n_active"] for q, ref in zip(qps, refs) if q.cls == "bigset"]
    assert big
    if P != "pendulum":
        assert sum(a >= 29 for a in big) >= max(1, len(big) // 4), big
    # zero-width boxes and weakly active bounds are really there
    for q, ref in zip(qps, refs):
        hi, lo = q.boxes()
        if q.name.startswith("zerowidth"):
            assert (hi[q.nx:] == lo[q.nx:]).sum() >= 3 * q.m.nu
        if q.name.startswith("weak"):
            at = (np.abs(ref["x"] - hi) < 1e-7) | (np.abs(ref["x"] - lo) < 1e-7)
            assert at[q.nx:].sum() >= 1 and not ref["strict"], q.name
    # +-1e20 and +-inf: the same optimum
    twins = {q.name: r for q, r in zip(qps, refs) if q.twin}
    a, b = list(twins.values())
    assert np.array_equal(a["x"], b["x"])
    # q scaled up and down: max(1, |q|inf) clamps to 1 in one copy and not in the other
    sc = {q.name: q.qscale() for q in qps if q.cls == "scaled"}
    assert sc["scaled-10000"] > 1.0 and sc["scaled-0.0001"] == 1.0


def test_reference_agrees_with_the_oracle_admm(plant):
    """On the feasible instances the dense interior point and the oracle's tight ADMM agree to 1e-6 wherever the ADMM converged."""
    from oracle import oracle as O
    P, qps, refs, lps = plant["model"], plant["qps"], plant["refs"], plant["lps"]
    compared = 0
    for q, ref, (t, verdict) in zip(qps, refs, lps):
        if ref is None or verdict != "feasible" or q.x0_violation() > 0.0:
            continue
        m = q.m
        d = O.dims_of(m.nx, m.nu, m.nw, q.N, m.ni, m.ni_f)
        l = np.where(np.isneginf(q.l), -1e20, q.l)
        u = np.where(np.isposinf(q.u), 1e20, np.where(np.isneginf(q.u), -1e20, q.u))
        x, y, info = O.qp_solve(d, q.A, q.B, m.G, m.Gf, m.Q, m.R, m.Qf, q.q, l, u, O.tight_settings())
        if info.status != 1:
            continue
        assert QC.relerr(x, ref["x"]) < 1e-6, (P, q.name)
        compared += 1
    assert compared >= 5, compared


def test_host_certificate_passes_the_optimum_and_fails_it_disturbed(plant):
    P, qps, refs = plant["model"], plant["qps"], plant["refs"]
    checked = 0
    for q, ref in zip(qps, refs):
        if ref is None or q.cls not in ("easy", "bigset", "stress"):
            continue
        x, y = ref["x"], ref["y"]
        ok, rep = QC.host_certificate(q, x, y, 0)
        assert ok, (P, q.name, rep)
        e = q.n // 2
        x1 = x.copy(); x1[e] += 1e-5 * max(1.0, abs(x[e]))
        assert not QC.host_certificate(q, x1, y, 0)[0], (P, q.name, "moved element")
        x2 = x.copy(); x2[e] = np.nan
        assert not QC.host_certificate(q, x2, y, 0)[0], (P, q.name, "NaN")
        y2 = y.copy(); y2[q.mb - 1] = np.nan
        assert not QC.host_certificate(q, x, y2, 0)[0], (P, q.name, "NaN multiplier")
        act = [r for i in range(q.nx, q.n) for r in (q.hi_row(i), q.lo_row(i)) if y[r] > 1e-6 * q.qscale()]
        if act:
            y3 = y.copy(); y3[act[0]] = -y3[act[0]]
            assert not QC.host_certificate(q, x, y3, 0)[0], (P, q.name, "multiplier of the wrong sign")
        checked += 1
    assert checked >= 4

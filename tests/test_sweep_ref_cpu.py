"""tests/sweep_ref.py (the plain np.longdouble restatement of the SLS sweep that tests/test_gpu_sweep_routes.py holds the HIP kernels against) is
itself pinned here, on the CPU: against the golden vectors of the reference's own kernels and against the C oracle, at the tolerances of
tests/test_oracle_sweep.py (1e-10 for K and the back-offs, 1e-9 for beta / beta_f, 1e-11 for Phi and S).  The input sets of the GPU tests
(tests/sweep_cases.py) are checked too: they can tell a wrong stage offset or a dropped disturbance column from the right answer, and the oracle
solves every instance of them.
"""
import glob
import os

import numpy as np
import pytest

import sweep_ref as SR
from conftest import GOLDEN
from oracle import oracle as O
from problems import oracle_dims, run_oracle_fastsls
from sweep_cases import ALL_CASES, B_MAX, case_id, make_case, shifted_E

GOLDEN_CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "sweep_*.npz")))
relerr = SR.relerr


def test_all_eight_golden_fixtures_are_present():
    assert len(GOLDEN_CASES) == 8


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_restatement_reproduces_the_reference_kernels(case):
    g = dict(np.load(os.path.join(GOLDEN, case)))
    N, nx = int(g["N"]), int(g["nx"])
    r = SR.sweep(g["A"], g["B"], g["E"], g["G"], g["Gf"], g["eta"], g["eta_f"], g["Q_reg"], g["R_reg"], g["Q_reg_f"], 1e-10)
    assert r["Phi_x"].shape == (N + 1, N + 1, nx, int(g["nw"]))
    assert relerr(r["K"], g["K"]) < 1e-10
    assert relerr(r["beta"], g["beta"]) < 1e-9
    assert relerr(r["beta_f"], g["beta_f"]) < 1e-9
    assert relerr(r["backoff"], g["backoff"]) < 1e-10
    assert relerr(r["backoff_f"], g["backoff_f"]) < 1e-10
    S, Px, Pu = (np.asarray(r[k], dtype=float) for k in ("S", "Phi_x", "Phi_u"))
    if "S" in g:
        assert relerr(S, g["S"]) < 1e-11
        assert relerr(Px, g["Phi_x"]) < 1e-11
        assert relerr(Pu, g["Phi_u"]) < 1e-11
        # cost_tube against SLS.eval_cost's definition on the reference's own Phi: || blkdiag(Q_reg.., Q_reg_f, R_reg..) [Phi_x; Phi_u] ||_F
        want = np.sqrt(sum(np.sum(((g["Q_reg"] if k < N else g["Q_reg_f"]) @ g["Phi_x"][k, j]) ** 2) for k in range(N + 1) for j in range(N + 1))
                       + sum(np.sum((g["R_reg"] @ g["Phi_u"][k, j]) ** 2) for k in range(N) for j in range(N + 1)))
        assert abs(float(r["cost_tube"]) - want) < 1e-11 * want
    else:           # the large fixtures hold block norms and a weighted checksum instead of the tensors
        w = np.cos(np.arange(nx * nx)).reshape(nx, nx)
        assert np.allclose(np.linalg.norm(S, axis=(2, 3)), g["S_fro"], rtol=1e-10, atol=0)
        assert np.allclose(np.einsum("kjab,ab->kj", S, w), g["S_chk"], rtol=1e-9, atol=1e-9 * np.abs(g["S_chk"]).max())
        assert np.allclose(np.linalg.norm(Px, axis=(2, 3)), g["Phix_fro"], rtol=1e-10, atol=1e-300)
        assert np.allclose(np.linalg.norm(Pu, axis=(2, 3)), g["Phiu_fro"], rtol=1e-9, atol=1e-300)


def test_quirk_q4_and_the_tightened_bounds_layout():
    """backoff_x[N] comes from backoff_f (q4); ubg = per stage [-c_k; g_k - backoff_k] without +eps (q3), then the raw gf - backoff_f (q2): the
    same vector OracleFastSLS.backward_and_tighten hands to its QP."""
    inst = make_case("pendulum", 2, "dense", 1)[0]
    m, N = inst.m, inst.N
    rng = np.random.default_rng(0)
    eta, eta_f = rng.uniform(0, 5, (N, N, m.ni)), rng.uniform(0, 5, (N + 1, m.ni_f))
    g = np.stack(inst.g_list[:N])
    r = SR.sweep(inst.A, inst.B, inst.E, m.G, m.Gf, eta, eta_f, m.Q_reg, m.R_reg, m.Q_reg_f, 1e-10, c=inst.c, g=g, gf_raw=m.gf)
    assert np.array_equal(r["backoff_x"][N], r["backoff_f"][: m.nx]) and np.array_equal(r["backoff_x"][:N], r["backoff"][:, : m.nx])
    assert np.array_equal(r["backoff_u"], r["backoff"][:, m.nx: m.nz])
    f = O.OracleFastSLS(oracle_dims(inst), m.G, m.Gf, m.g, m.gf, inst.E, m.Q, m.R, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f)
    f.update_dynamics_list(inst.A, inst.B, inst.E, inst.g_list, inst.c)
    f.cur["eta"], f.cur["eta_f"] = eta, eta_f
    f.backward_and_tighten()
    assert r["ubg"].shape == f.qp.ubg.shape and relerr(r["ubg"], f.qp.ubg) < 1e-12
    assert relerr(r["backoff_x"], f.cur["backoff_x"]) < 1e-10


def _random_eta(inst, seed):
    """A full per-column eta of the size the solver produces: mu / (2 sqrt(beta)) with mu mostly zero (inactive rows)."""
    m, N = inst.m, inst.N
    rng = np.random.default_rng(seed)
    eta = rng.uniform(0, 3e3, (N, N, m.ni)) * (rng.uniform(size=(N, N, m.ni)) < 0.3)
    eta_f = rng.uniform(0, 3e3, (N + 1, m.ni_f)) * (rng.uniform(size=(N + 1, m.ni_f)) < 0.3)
    return eta, eta_f


@pytest.mark.parametrize("model,N,variant", ALL_CASES, ids=[case_id(*c) for c in ALL_CASES])
def test_restatement_agrees_with_the_oracle_and_the_inputs_discriminate(model, N, variant):
    inst = make_case(model, N, variant, 1)[0]
    m = inst.m
    d = oracle_dims(inst)
    assert inst.E.shape == (N + 1, m.nx, m.nw) and (m.nw < m.nx) == (variant == "nw")
    if variant != "model":
        assert all(np.count_nonzero(inst.E[j]) > m.nx for j in range(1, N + 1))                  # dense ...
        assert all(not np.array_equal(inst.E[j], inst.E[j + 1]) for j in range(N))               # ... and different at every stage
    for eta, eta_f in (_random_eta(inst, 3), (np.zeros((N, N, m.ni)), np.zeros((N + 1, m.ni_f)))):
        r = SR.sweep(inst.A, inst.B, inst.E, m.G, m.Gf, eta, eta_f, m.Q_reg, m.R_reg, m.Q_reg_f, 1e-10)
        S, K = O.backward(d, inst.A, inst.B, m.G, m.Gf, eta, eta_f, m.Q_reg, m.R_reg, m.Q_reg_f)
        Px, Pu = O.propagate(d, inst.A, inst.B, inst.E, K)
        beta, beta_f, bo, bof = O.backoff(d, Px, Pu, m.G, m.Gf, 1e-10)
        assert relerr(K, r["K"]) < 1e-10 and relerr(S, r["S"]) < 1e-11
        assert relerr(Px, r["Phi_x"]) < 1e-11 and relerr(Pu, r["Phi_u"]) < 1e-11
        assert relerr(beta, r["beta"]) < 1e-9 and relerr(beta_f, r["beta_f"]) < 1e-9
        assert relerr(bo, r["backoff"]) < 1e-10 and relerr(bof, r["backoff_f"]) < 1e-10
        assert all(not r["beta"][k, j].any() and not r["K"][k, j].any() for k in range(N) for j in range(k + 1, N))
        if variant == "model":
            continue
        # a wrong stage offset (E_{j+1} for column j) and, with nw < nx, a lost last column must be far outside the 1e-9 the GPU tests allow
        wrong = SR.sweep(inst.A, inst.B, shifted_E(inst.E), m.G, m.Gf, eta, eta_f, m.Q_reg, m.R_reg, m.Q_reg_f, 1e-10)
        assert relerr(wrong["beta"], r["beta"]) > 1e-3 and relerr(wrong["beta_f"], r["beta_f"]) > 1e-3
        if variant == "nw":
            E0 = inst.E.copy()
            E0[:, :, -1] = 0.0
            wrong = SR.sweep(inst.A, inst.B, E0, m.G, m.Gf, eta, eta_f, m.Q_reg, m.R_reg, m.Q_reg_f, 1e-10)
            assert relerr(wrong["beta"], r["beta"]) > 1e-3 and relerr(wrong["beta_f"], r["beta_f"]) > 1e-3


@pytest.mark.parametrize("model,N,variant", ALL_CASES, ids=[case_id(*c) for c in ALL_CASES])
def test_the_oracle_solves_every_instance_of_every_input_set(model, N, variant, monkeypatch):
    """Two fast-SLS steps (QP, sweep, tightened QP, sweep, tightened QP) of the CPU oracle at its tight settings, with the convergence test
    switched off (what opts.conv_tol = -1 does on the GPU), succeed on all 11 instances, every QP included -- the first step is what rti_steps = 1
    runs -- so the GPU tests can demand a swept, successful result from every instance.  The inputs have active constraints: eta is not zero among
    the first three instances (the batch of the small GPU cases), and after the second iteration it differs between columns 0 and N - 1 of the
    last stage for some instance."""
    monkeypatch.setattr(O.OracleFastSLS, "check_convergence", lambda self: False)
    nonzero, differs = [], []
    for b, inst in enumerate(make_case(model, N, variant, B_MAX)):
        out = run_oracle_fastsls(inst, rti_steps=2)          # (a QP that fails ends the loop early: iteration_number stays below 2)
        assert out["success"] and out["iteration_number"] == 2 and out["_qp_info"].status == 1, (b, out["_qp_info"].status)
        nonzero.append(bool(out["eta"].any()))
        differs.append(bool((out["eta"][N - 1, 0] != out["eta"][N - 1, N - 1]).any()))
    assert any(nonzero[:3])
    assert any(differs) or N == 1          # (N = 1: the two are the same entry)

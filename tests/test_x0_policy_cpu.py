"""The x0-tolerance option (slsqp_set_x0_box_tol) where no device is needed: what the reference's OSQP settings do with a measured state outside
its stage-0 box (the measurement behind X0_BOX_TOL_OSQP_DEFAULT), the recorded violations of the script-regime closed loop, and the plumbing."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import x0_policy as XP
from conftest import GOLDEN


@pytest.fixture(scope="module")
def acceptance():
    return XP.osqp_acceptance()


def test_osqp_default_settings_acceptance_of_x0_violations(acceptance):
    """The oracle's OSQP restatement at O.default_settings() on the x0-edge QPs (three plants, seeds 40-43) over 17 violations from 1e-5 to 1e-1.
    Measured (accepted = status 1 or 2, of 12):
        1e-5 ... 1.778e-3: 12 each | 3.162e-3: 8 | 5.623e-3: 1 | 1e-2 ... 1e-1: 0       (every accepted solve: status 1, polished, pri_res = violation / 2;
                                                                                         every other one: primal infeasible)"""
    from robust_nonlinear_mpc_amd import X0_BOX_TOL_OSQP_DEFAULT
    n, M = XP.accepted_table(acceptance)
    print("violation        :", " ".join(f"{g:9.3e}" for g in XP.GRID))
    print("accepted (of %2d) :" % M.shape[0], " ".join(f"{v:9d}" for v in n))
    for (P, s), rows in acceptance.items():
        print(f"{P:9s} {s}:", " ".join(f"{st:3d}/{pol:1d}/{r:7.1e}" for st, pol, r in rows))
    assert len(XP.GRID) >= 9 and XP.GRID[0] == 1e-5 and XP.GRID[-1] == 1e-1 and M.shape[0] >= 12
    # (a) monotone along the grid: a QP refused at one violation is refused at every larger one, up to one plant-seed exception per grid point
    for j in range(1, len(XP.GRID)):
        regained = int(np.sum(M[:, j] & ~M[:, :j].all(axis=1)))
        assert regained <= 1, (XP.GRID[j], regained)
    # (b) everything accepted at the two smallest violations, nothing at the largest
    assert M[:, 0].all() and M[:, 1].all() and not M[:, -1].any()
    # (c) the constant lies where every QP was accepted
    all_ok = [g for j, g in enumerate(XP.GRID) if M[:, :j + 1].all()]
    assert X0_BOX_TOL_OSQP_DEFAULT <= max(all_ok), (X0_BOX_TOL_OSQP_DEFAULT, all_ok)
    assert X0_BOX_TOL_OSQP_DEFAULT > 1e-9


def test_recorded_closed_loop_violations_are_consistent():
    """tests/golden/x0_violation_rocket_script.npz: the strict 64-seed x 30-step rocket loop from the script's x0 as the MI355X ran it (seed, step,
    slot, violation, status per QP; scripts/x0_policy.py --record).  A solve that took part is refused exactly when its violation exceeds 1e-9."""
    d = np.load(os.path.join(GOLDEN, "x0_violation_rocket_script.npz"))
    seed, step, slot, viol, status = (d[k] for k in ("seed", "step", "slot", "violation", "status"))
    assert seed.shape == step.shape == slot.shape == viol.shape == status.shape == (64 * 30 * 2,)
    assert len(set(zip(seed.tolist(), step.tolist(), slot.tolist()))) == 64 * 30 * 2
    assert set(seed.tolist()) == set(range(64)) and set(step.tolist()) == set(range(30)) and set(slot.tolist()) == {0, 1}
    part = status != -1
    assert np.array_equal(status[part] == 2, viol[part] > 1e-9)
    assert (viol[~part] == 0.0).all()                       # a QP that took no part records no violation
    assert (status == 2).any() and np.isfinite(viol).all()
    # QP #2 takes no part exactly where QP #1 did not end on a solution
    s0 = {(a, b): st for a, b, sl, st in zip(seed.tolist(), step.tolist(), slot.tolist(), status.tolist()) if sl == 0}
    for a, b, sl, st in zip(seed.tolist(), step.tolist(), slot.tolist(), status.tolist()):
        if sl == 1:
            assert (st == -1) == (s0[(a, b)] not in (0, 4)), (a, b, st, s0[(a, b)])


def test_option_plumbing_without_a_device(tmp_path):
    import robust_nonlinear_mpc_amd as pkg
    from robust_nonlinear_mpc_amd import _lib as L, can_run_persistent, get_model
    from robust_nonlinear_mpc_amd.closed_loop import ClosedLoopMPC
    assert pkg.X0_BOX_TOL_OSQP_DEFAULT == L.X0_BOX_TOL_OSQP_DEFAULT and 1e-9 < L.X0_BOX_TOL_OSQP_DEFAULT <= 1e-2
    # the option is a property of the handle (slsqp_set_x0_box_tol): slsqp_opts and its mirror keep their layout, the mirror of a handle's options
    # carries it as a Python property on top of the same struct
    assert "x0_box_tol" not in [n for n, _ in L.Opts._fields_] and C.sizeof(L.HandleOpts) == C.sizeof(L.Opts)
    assert isinstance(L.HandleOpts.x0_box_tol, property) and {"slsqp_set_x0_box_tol", "slsqp_get_x0_box_tol"} <= set(L.EXPORTS)
    assert re.search(r"\bint\s+slsqp_set_x0_box_tol\s*\(\s*slsqp_handle\s*\*\s*h\s*,\s*double\s+tol\s*\)\s*;", re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "slsqp.h")).read(), flags=re.S))
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "slsqp.h")).read()
    assert float(re.search(r"#define SLSQP_X0_BOX_TOL_OSQP_DEFAULT\s+(\S+)", hdr).group(1)) == L.X0_BOX_TOL_OSQP_DEFAULT      # header and mirror agree
    # the persistent launch takes every tolerance
    for rti, steps in ((1, 1), (3, 2), (-1, 1), (1, None)):
        base = can_run_persistent(rti, steps, L.Opts(precision=0, fuse_rti=1), environ={})
        for tol in (0.0, L.X0_BOX_TOL_OSQP_DEFAULT, float("inf")):
            assert can_run_persistent(rti, steps, types.SimpleNamespace(precision=0, fuse_rti=1, x0_box_tol=tol), environ={}) == base
    # save_npz writes the reference's key set, whatever else the result dictionary holds
    m, N, steps = get_model("rocket"), 5, 4
    out = dict(state_trajectory=np.zeros((2, m.nx, steps)), input_trajectory=np.zeros((2, m.nu, steps - 1)),
               nominal_trajectory_x=np.zeros((2, m.nx, N + 1, steps)), nominal_trajectory_u=np.zeros((2, m.nu, N, steps)),
               backoff_trajectory_x=np.zeros((2, m.nx, N + 1, steps)), backoff_trajectory_u=np.zeros((2, m.nu, N, steps)),
               t_jac=np.zeros((steps, 1)), t_qp=np.zeros((steps, 1)), t_riccati=np.zeros((steps, 1)), success=np.ones((2, steps), dtype=bool))
    stub = types.SimpleNamespace(m=m, N=N)
    ClosedLoopMPC.save_npz(stub, str(tmp_path / "a.npz"), out, 1)
    ClosedLoopMPC.save_npz(stub, str(tmp_path / "b.npz"), dict(out, x0_violation=np.zeros((2, steps, 2)), qp_stats=np.zeros((2, steps, 2, 8), dtype=np.int32)), 1)
    ka, kb = sorted(np.load(tmp_path / "a.npz").files), sorted(np.load(tmp_path / "b.npz").files)
    assert ka == kb == sorted(["state_trajectory", "input_trajectory", "nominal_trajectory_x", "nominal_trajectory_u", "backoff_trajectory_x",
                               "backoff_trajectory_u", "dt", "g", "nx", "nu", "simulation_time_steps", "N", "t_jac", "t_qp", "t_riccati"])


def test_gate_rule_and_relaxed_qp():
    """the helpers the GPU tests judge the kernel with: max(1e-9, tol), inf never refuses a finite violation, NaN / inf states always refused"""
    import qp_corpus as QC
    assert not XP.gate(5e-10, 0.0) and XP.gate(1e-6, 0.0) and not XP.gate(1e-6, 1e-3) and XP.gate(2e-3, 1e-3)
    assert not XP.gate(1.0, np.inf) and XP.gate(np.inf, np.inf) and XP.gate(np.nan, np.inf) and not XP.gate(-0.3, 0.0)
    qp = QC._x0edge("pendulum", 42, 1e-3)
    r = XP.relaxed(qp)
    assert abs(qp.x0_violation() - 1e-3) < 1e-15 and r.x0_violation() < -1e19
    hi, lo = r.boxes()
    hi0, lo0 = qp.boxes()
    assert np.array_equal(hi[qp.nx:], hi0[qp.nx:]) and np.array_equal(lo[qp.nx:], lo0[qp.nx:])     # only the stage-0 state rows moved
    assert QC.reference(qp) is None and QC.reference(r) is not None

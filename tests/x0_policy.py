"""Helpers shared by the x0-tolerance tests and scripts/x0_policy.py (CPU only, no GPU library needed to import).

The tolerance mode (slsqp_set_x0_box_tol) accepts a QP whose pinned x_0 lies a little outside its own stage-0 box and then returns the
optimum of the QP WITHOUT its stage-0 state rows.  `relaxed` builds that QP, `osqp_acceptance` runs the oracle's OSQP restatement at the
reference's live settings on the x0-edge QPs of tests/qp_corpus.py, `tolerant_backend` is the closed-loop oracle's exact QP solver under the
same policy.
"""
import numpy as np

import qp_corpus as QC

# geometric grid of stage-0 violations, four points per decade from 1e-5 to 1e-1
GRID = tuple(float(f"{v:.4g}") for v in 10.0 ** (np.arange(-20, -3) / 4.0))
SEEDS = (40, 41, 42, 43)


def relaxed(qp):
    """copy of `qp` with its stage-0 state rows set to +-1e20 (no bound): the QP an accepted solve answers"""
    c = qp.copy(name=qp.name + "-relaxed")
    for i in range(qp.nx):
        c.set_box(i, hi=1e20, lo=-1e20)
    return c


def gate(violation, tol):
    """the kernel's rule: refused (status 2) iff the violation exceeds max(1e-9, tol); a NaN / infinite violation is always refused"""
    return bool(violation > max(1e-9, tol)) or not bool(violation < np.inf)


def osqp_acceptance(grid=GRID, seeds=SEEDS, plants=QC.PLANTS):
    """status of the oracle's OSQP restatement at O.default_settings() (eps_abs = eps_rel = 1e-3, polish on: the reference's live settings,
    qp_jit.py:537-548) on `qp_corpus._x0edge(model, seed, off)` for every off of the grid.  Returns dict (plant, seed) -> list of
    (status, polish_status, pri_res) along the grid."""
    from oracle import oracle as O
    out = {}
    for P in plants:
        for s in seeds:
            rows = []
            for off in grid:
                qp = QC._x0edge(P, s, off)
                m = qp.m
                d = O.dims_of(m.nx, m.nu, m.nw, qp.N, m.ni, m.ni_f)
                _, _, info = O.qp_solve(d, qp.A, qp.B, m.G, m.Gf, m.Q, m.R, m.Qf, qp.q, qp.l, qp.u, O.default_settings())
                rows.append((int(info.status), int(info.polish_status), float(info.pri_res)))
            out[(P, s)] = rows
    return out


def accepted_table(acc):
    """(n_grid,) number of QPs that came back 'solved' or 'solved inaccurate' (status 1 / 2: what qp_jit.py:397 accepts) per grid point, and the
    boolean matrix (n_qps, n_grid) behind it"""
    M = np.array([[st in (1, 2) for st, _, _ in rows] for rows in acc.values()])
    return M.sum(axis=0), M


def tolerant_backend(tol, seen=None):
    """QP back end for tests/problems.run_oracle_closed_loop (`fs.qp.backend`) under the tolerance policy: when the pinned x_0 lies within
    max(1e-9, tol) of its stage-0 box, the stage-0 state rows of u are widened to 1e20 and problems.ipm_backend solves the rest unchanged
    (beyond the tolerance ipm_backend refuses the QP as it always does).  `seen`: list that receives every violation met."""
    from problems import ipm_backend

    def backend(qp, l, u):
        d = qp.d
        nx, nz = d.nx, d.nx + d.nu
        x0val = 0.5 * (l[-nx:] + u[-nx:])
        viol = float(np.max(np.maximum(x0val - u[nx:2 * nx], -u[nx + nz:nx + nz + nx] - x0val)))
        if seen is not None:
            seen.append(viol)
        if not gate(viol, tol):
            u = u.copy()
            u[nx:2 * nx] = 1e20
            u[nx + nz:nx + nz + nx] = 1e20
        return ipm_backend(qp, l, u)
    return backend

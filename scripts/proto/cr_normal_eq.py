"""Block cyclic reduction of the solver's normal equations  Y nu = b  in numpy, next to the sequential block LDL' recursion and a dense solve.

The prototype of csrc/slsqp_mw.hpp (ne_solve_cr), in that routine's order of operations, and the yardstick of its tests:

    Y_kk      = A_k diag(pi_x,k) A_k' [k > 0] + B_k diag(pi_u,k) B_k' + diag(pi_x,k+1) + delta
    Y_{k,k-1} = -A_k diag(pi_x,k)

  sequential   D_k = Y_kk - O_k D_{k-1}^-1 O_k',  forward elimination, backward substitution  (ne_forward / ne_backward)
  cyclic       level s = 1, 2, 4, ..: the list holds the blocks 0, s, 2s, ..; block i = (2m+1) s is eliminated against l = i - s and r = i + s:
                 F_l = D_i^-1 Y_{i,l},  F_r = D_i^-1 Y_{i,r},  y_i = D_i^-1 b_i,
                 D_l -= Y_{i,l}' F_l,  b_l -= F_l' b_i,   D_r -= Y_{r,i} F_r,  b_r -= F_r' b_i,   Y_{r,l} = -Y_{r,i} F_l;
               block 0 is the root; back-substitution nu_i = y_i - F_l nu_l - F_r nu_r down the levels.
               `cr_factor` keeps D_i^-1, F_l, F_r; `cr_solve` substitutes with them alone (what a solve-only tick of the kernel does).

Run as a script it prints, per plant and weighting, the worst relative residual (long double) of the three solvers over the QPs of
tests/qp_corpus.py that have a reference optimum:   python scripts/proto/cr_normal_eq.py [plant ...]
"""
import os
import sys

import numpy as np

DELTA = 1e-13
WEIGHTINGS = ("active-set", "late-ipm", "mid-ipm")


def stage_blocks(A, B, pi, delta=DELTA):
    """Diagonal blocks D (N,nx,nx) and sub-diagonal couplings C (N,nx,nx; C[0] unused) of Y from A (N,nx,nx), B (N,nx,nu), pi (n)."""
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    nz = nx + nu
    D, Cc = np.zeros((N, nx, nx)), np.zeros((N, nx, nx))
    for k in range(N):
        px, pu, pn = pi[k * nz:k * nz + nx], pi[k * nz + nx:(k + 1) * nz], pi[(k + 1) * nz:(k + 1) * nz + nx]
        D[k] = (B[k] * pu) @ B[k].T + np.diag(pn + delta)
        if k > 0:
            D[k] += (A[k] * px) @ A[k].T
            Cc[k] = -A[k] * px
    return D, Cc


def rhs(A, B, v):
    """b_k = A_k v_x,k + B_k v_u,k - v_x,k+1"""
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    nz = nx + nu
    return np.stack([A[k] @ v[k * nz:k * nz + nx] + B[k] @ v[k * nz + nx:(k + 1) * nz] - v[(k + 1) * nz:(k + 1) * nz + nx] for k in range(N)])


def E_t_nu(A, B, nu):
    """G = E' nu in the layout of the solver's n-vectors"""
    N, nx, nu_ = A.shape[0], A.shape[1], B.shape[2]
    nz = nx + nu_
    G = np.zeros(nz * N + nx)
    for k in range(N):
        G[k * nz:k * nz + nx] += A[k].T @ nu[k]
        G[k * nz + nx:(k + 1) * nz] = B[k].T @ nu[k]
        G[(k + 1) * nz:(k + 1) * nz + nx] -= nu[k]
    return G


def dense(D, Cc):
    N, nx = D.shape[0], D.shape[1]
    Y = np.zeros((N * nx, N * nx))
    for k in range(N):
        Y[k * nx:(k + 1) * nx, k * nx:(k + 1) * nx] = D[k]
        if k > 0:
            Y[k * nx:(k + 1) * nx, (k - 1) * nx:k * nx] = Cc[k]
            Y[(k - 1) * nx:k * nx, k * nx:(k + 1) * nx] = Cc[k].T
    return Y


def residual(D, Cc, b, nu):
    """relative residual |Y nu - b|inf / |b|inf, accumulated in long double"""
    L = np.longdouble
    N = D.shape[0]
    Dl, Cl, bl, nl = D.astype(L), Cc.astype(L), b.astype(L), nu.astype(L)
    r = np.zeros_like(bl)
    for k in range(N):
        r[k] = Dl[k] @ nl[k] - bl[k]
        if k > 0:
            r[k] += Cl[k] @ nl[k - 1]
        if k + 1 < N:
            r[k] += Cl[k + 1].T @ nl[k + 1]
    return float(np.abs(r).max() / max(float(np.abs(bl).max()), 1e-300))


def seq_solve(D, Cc, b):
    """sequential block LDL' with explicit inverses (the single-wave kernels' sweeps)"""
    N = D.shape[0]
    Dinv, u = np.zeros_like(D), np.zeros_like(b)
    for k in range(N):
        Dk, t = D[k].copy(), b[k].copy()
        if k > 0:
            T = Cc[k] @ Dinv[k - 1]
            Dk -= T @ Cc[k].T
            t -= Cc[k] @ u[k - 1]
        Dinv[k] = np.linalg.inv(Dk)
        Dinv[k] = 0.5 * (Dinv[k] + Dinv[k].T)
        u[k] = Dinv[k] @ t
    nu = u.copy()
    for k in range(N - 2, -1, -1):
        nu[k] = u[k] - Dinv[k] @ (Cc[k + 1].T @ nu[k + 1])
    return nu


def _levels(N):
    s = 1
    while s < N:
        yield s, [(2 * m + 1) * s for m in range(((N + s - 1) // s) // 2)]
        s *= 2


def cr_factor(D, Cc):
    """-> F (N,3,nx,nx): D_i^-1, F_l, F_r of every eliminated block, the root's inverse in F[0,0]; ok = every block was positive definite"""
    N, nx = D.shape[0], D.shape[1]
    D, Cc = D.copy(), Cc.copy()          # Cc[j]: coupling of block j to its left neighbour in the current list
    F = np.zeros((N, 3, nx, nx))
    ok = True

    def inv(M):
        nonlocal ok
        M = np.tril(M) + np.tril(M, -1).T          # (the kernel reads the lower triangle)
        ok = ok and bool(np.all(np.linalg.eigvalsh(M) > 0))
        # (np.linalg.inv as it comes: averaging it with its transpose costs the small residual D_i D_i^-1 - I that LAPACK's inverse has, and with it
        #  a factor 10 - 30 in the residual of the whole solve on the rocket's systems)
        return np.linalg.inv(M)
    for s, elim in _levels(N):
        new = []
        for i in elim:
            l, r = i - s, i + s
            Di = inv(D[i])
            F[i, 0], F[i, 1] = Di, Di @ Cc[i]
            D[l] -= Cc[i].T @ F[i, 1]
            if r < N:
                F[i, 2] = Di @ Cc[r].T
                new.append((r, Cc[r] @ F[i, 2], -Cc[r] @ F[i, 1]))
        for r, dD, Cr in new:          # (the kernel updates the right neighbours behind a barrier)
            D[r] -= dD
            Cc[r] = Cr
    F[0, 0] = inv(D[0])
    return F, ok


def cr_solve(F, b):
    """substitution with the stored factors alone"""
    N = F.shape[0]
    lv = list(_levels(N))
    y = b.copy()
    for s, elim in lv:
        saved = {i: y[i].copy() for i in elim}
        for i in elim:
            y[i] = F[i, 0] @ saved[i]
            y[i - s] -= F[i, 1].T @ saved[i]
        for i in elim:
            if i + s < N:
                y[i + s] -= F[i, 2].T @ saved[i]
    y[0] = F[0, 0] @ y[0]
    for s, elim in reversed(lv):
        for i in elim:
            y[i] -= F[i, 1] @ y[i - s]
            if i + s < N:
                y[i] -= F[i, 2] @ y[i + s]
    return y


def cr(D, Cc, b):
    F, ok = cr_factor(D, Cc)
    return cr_solve(F, b), ok


# ---- the corpus systems ---------------------------------------------------------------------------------------------
def active_mask(qp, ref):
    """elements the reference optimum holds at a bound (its multipliers), x_0 (pinned) included"""
    y, sc = ref["y"], qp.qscale()
    idx = np.arange(qp.n)
    lu, ll = y[[qp.hi_row(e) for e in idx]], y[[qp.lo_row(e) for e in idx]]
    act = (lu > 1e-6 * sc) | (ll > 1e-6 * sc)
    act[:qp.nx] = True
    return act


def weighting(qp, act, which):
    """Pi of an active-set round at the optimal set / of a late / mid interior-point iteration (w: barrier weight on active, inactive elements)"""
    P = qp.Pd()
    if which == "active-set":
        pi = np.where(act, 0.0, 1.0 / P)
    else:
        wa, wi = (1e8, 1e-8) if which == "late-ipm" else (1e3, 1e-2)
        pi = 1.0 / (P + np.where(act, wa, wi) * qp.qscale())
    pi[:qp.nx] = 0.0
    return pi


def system(qp, act, which, N=None):
    """D, C of the QP's normal equations with the horizon cut to N stages, and the weights"""
    N = qp.N if N is None else N
    nz = qp.nz
    pi = weighting(qp, act, which)[:nz * N + qp.nx]
    D, Cc = stage_blocks(qp.A[:N], qp.B[:N], pi)
    return D, Cc, pi


def main(plants):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
    import qp_corpus as QC
    print(f"{'plant':10s} {'weighting':11s} {'cond max':>9s} {'sequential':>11s} {'cyclic':>11s} {'worst ratio':>11s}")
    for plant in plants:
        qps = QC.corpus(plant)
        refs = [QC.reference(q) for q in qps]
        rng = np.random.default_rng(1)
        for which in WEIGHTINGS:
            worst = [0.0, 0.0, 0.0, 0.0]
            for qp, ref in zip(qps, refs):
                if ref is None:
                    continue
                D, Cc, _ = system(qp, active_mask(qp, ref), which)
                b = rng.normal(size=(qp.N, qp.nx))
                rs, rc = residual(D, Cc, b, seq_solve(D, Cc, b)), residual(D, Cc, b, cr(D, Cc, b)[0])
                worst = [max(worst[0], np.linalg.cond(dense(D, Cc))), max(worst[1], rs), max(worst[2], rc), max(worst[3], rc / rs)]
            print(f"{plant:10s} {which:11s} {worst[0]:9.1e} {worst[1]:11.2e} {worst[2]:11.2e} {worst[3]:11.2f}")


if __name__ == "__main__":
    main(sys.argv[1:] or ["pendulum", "quadrotor", "rocket"])

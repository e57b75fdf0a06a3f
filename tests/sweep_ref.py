"""Plain np.longdouble restatement of the SLS sweep (test helper, CPU only): loops and `@`, nothing else.

What it restates (the reference's solver/fast_SLS_jit.py:65-188 and 489-571, util/SLS.py:38-46; the project's CPU oracle has the same three
functions in C, oracle/sls_oracle.c):

  backward    per disturbance column j the Riccati recursion  S[N,j] = Gf' diag(eta_f[j]) Gf + Q_reg_f,  C = G' diag(eta[k,j]) G,
              K[k,j] = -(C_uu + R_reg + B' S B)^-1 B' S A,  S[k,j] = sym(C_xx + Q_reg + A' S (A + B K))            k = N-1 .. j
  propagate   Phi_x[j,j] = E_j,  Phi_u[k,j] = K[k,j] Phi_x[k,j],  Phi_x[k+1,j] = (A_k + B_k K[k,j]) Phi_x[k,j]       k = j .. N-1
  backoff     beta[k,j,i] = max(|| G_i [Phi_x[k,j]; Phi_u[k,j]] ||^2, eps) (j <= k, 0 above the diagonal), beta_f[j,i] likewise with Gf and
              Phi_x[N,j]; backoff[k] = sum_{j<=k} sqrt(beta[k,j]), backoff_f = sum_j sqrt(beta_f[j]);
              backoff_x = [backoff[:, :nx]; backoff_f[:nx]] (quirk q4: the last row comes from backoff_f), backoff_u = backoff[:, nx:nx+nu]
  cost_tube   || blkdiag(Q_reg x N, Q_reg_f, R_reg x N) [Phi_x; Phi_u] ||_F
  ubg         per stage [-c_k; g_k - backoff_k] (no +eps: quirk q3), then gf_raw - backoff_f (the model's raw gf: quirk q2)

General G and Gf, any nw, one E block per stage.  Everything is computed in np.longdouble and returned in that type; callers compare
float64 results against it.
"""
import numpy as np

LD = np.longdouble


def _ld(a):
    return np.array(a, dtype=LD)


def _solve(H, F):
    """H Z = F by Gaussian elimination with partial pivoting (np.linalg has no longdouble)."""
    n = H.shape[0]
    a, z = H.copy(), F.copy()
    for c in range(n):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        if p != c:
            a[[c, p]] = a[[p, c]]
            z[[c, p]] = z[[p, c]]
        for r in range(c + 1, n):
            f = a[r, c] / a[c, c]
            a[r] = a[r] - f * a[c]
            z[r] = z[r] - f * z[c]
    for r in range(n - 1, -1, -1):
        z[r] = (z[r] - a[r, r + 1:] @ z[r + 1:]) / a[r, r]
    return z


def backward(A, B, G, Gf, eta, eta_f, Q_reg, R_reg, Q_reg_f):
    A, B, G, Gf, eta, eta_f, Q_reg, R_reg, Q_reg_f = map(_ld, (A, B, G, Gf, eta, eta_f, Q_reg, R_reg, Q_reg_f))
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    S = np.zeros((N + 1, N + 1, nx, nx), dtype=LD)
    K = np.zeros((N, N + 1, nu, nx), dtype=LD)
    for j in range(N + 1):
        S[N, j] = Gf.T @ (eta_f[j][:, None] * Gf) + Q_reg_f
        for k in range(N - 1, j - 1, -1):
            C = G.T @ (eta[k, j][:, None] * G)
            Sn = S[k + 1, j]
            x = B[k].T @ Sn
            y = A[k].T @ Sn
            H = C[nx:, nx:] + R_reg + x @ B[k]
            K[k, j] = -_solve(H, x @ A[k])
            Sk = C[:nx, :nx] + Q_reg + y @ (A[k] + B[k] @ K[k, j])
            S[k, j] = (Sk + Sk.T) / 2
    return S, K


def propagate(A, B, E, K):
    A, B, E, K = map(_ld, (A, B, E, K))
    N, nx, nu, nw = A.shape[0], A.shape[1], B.shape[2], E.shape[2]
    Px = np.zeros((N + 1, N + 1, nx, nw), dtype=LD)
    Pu = np.zeros((N, N + 1, nu, nw), dtype=LD)
    for j in range(N + 1):
        Px[j, j] = E[j]
        for k in range(j, N):
            Pu[k, j] = K[k, j] @ Px[k, j]
            Px[k + 1, j] = (A[k] + B[k] @ K[k, j]) @ Px[k, j]
    return Px, Pu


def backoff(Px, Pu, G, Gf, eps=1e-10):
    Px, Pu, G, Gf = map(_ld, (Px, Pu, G, Gf))
    N, nx, nu = Pu.shape[0], Px.shape[2], Pu.shape[2]
    ni, nif = G.shape[0], Gf.shape[0]
    eps = LD(eps)
    beta = np.zeros((N, N, ni), dtype=LD)
    beta_f = np.zeros((N + 1, nif), dtype=LD)
    for k in range(N):
        for j in range(k + 1):
            rows = G @ np.vstack([Px[k, j], Pu[k, j]])
            for i in range(ni):
                beta[k, j, i] = max(rows[i] @ rows[i], eps)
    for j in range(N + 1):
        rows = Gf @ Px[N, j]
        for i in range(nif):
            beta_f[j, i] = max(rows[i] @ rows[i], eps)
    bo = np.zeros((N, ni), dtype=LD)
    for k in range(N):
        for j in range(k + 1):
            bo[k] = bo[k] + np.sqrt(beta[k, j])
    bof = np.zeros(nif, dtype=LD)
    for j in range(N + 1):
        bof = bof + np.sqrt(beta_f[j])
    bx = np.vstack([bo[:, :nx], bof[:nx]])
    bu = bo[:, nx:nx + nu].copy()
    return dict(beta=beta, beta_f=beta_f, backoff=bo, backoff_f=bof, backoff_x=bx, backoff_u=bu)


def cost_tube(Px, Pu, Q_reg, R_reg, Q_reg_f):
    Px, Pu, Q_reg, R_reg, Q_reg_f = map(_ld, (Px, Pu, Q_reg, R_reg, Q_reg_f))
    N = Pu.shape[0]
    acc = LD(0)
    for j in range(N + 1):
        for k in range(N + 1):
            W = (Q_reg if k < N else Q_reg_f) @ Px[k, j]
            acc = acc + (W * W).sum()
        for k in range(N):
            W = R_reg @ Pu[k, j]
            acc = acc + (W * W).sum()
    return np.sqrt(acc)


def tightened_ubg(c, g, gf_raw, bo, bof):
    c, g, gf_raw, bo, bof = map(_ld, (c, g, gf_raw, bo, bof))
    rows = []
    for k in range(c.shape[0]):
        rows.append(-c[k])
        rows.append(g[k] - bo[k])
    rows.append(gf_raw - bof)
    return np.concatenate(rows)


def sweep(A, B, E, G, Gf, eta, eta_f, Q_reg, R_reg, Q_reg_f, eps=1e-10, c=None, g=None, gf_raw=None):
    """The whole sweep on one instance.  Returns S, K, Phi_x, Phi_u, beta, beta_f, backoff, backoff_f, backoff_x, backoff_u, cost_tube and, when
    c (N,nx), g (N,ni) and gf_raw (ni_f) are given, the tightened ubg."""
    S, K = backward(A, B, G, Gf, eta, eta_f, Q_reg, R_reg, Q_reg_f)
    Px, Pu = propagate(A, B, E, K)
    out = backoff(Px, Pu, G, Gf, eps)
    out.update(S=S, K=K, Phi_x=Px, Phi_u=Pu, cost_tube=cost_tube(Px, Pu, Q_reg, R_reg, Q_reg_f))
    if c is not None:
        out["ubg"] = tightened_ubg(c, g, gf_raw, out["backoff"], out["backoff_f"])
    return out


def relerr(a, b):
    """Max-norm relative error of a against the reference b (the project's sweep measure)."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / max(LD(1e-300), np.max(np.abs(b))))

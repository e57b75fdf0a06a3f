"""Plain numpy restatement of a hold step (test helper, CPU only): the tube's disturbance-feedback policy between two solves, in its column
(state-space) realisation of Phi_u = K Phi_x (the reference's solver/fast_SLS_jit.py:87-117), and the plant step after it.

Hold step k after a solve that pinned stage 0 of the plan to the measured state; z_k, v_k the plan's nominal at stage k; A_j, B_j, K[k,j] as
the solve left them; column states xi_j (nx):

    e     = x_meas - z_k
    xi_j <- (A_{k-1} + B_{k-1} K[k-1,j]) xi_j        first <= j < k
    xi_k  = e - sum_{j<k} xi_j
    u     = v_k + sum_{first<=j<=k} K[k,j] xi_j
    x_meas <- plant(x_meas, u) + E w

On the device column 0 is zero because x_0 is pinned (first = 1, k >= 1).  first = 0 admits a non-zero column 0 and k = 0: the realisation of the
whole disturbance response, which tests/test_hold_cpu.py holds against the reference's Phi_x / Phi_u.
"""
import numpy as np


def policy(k, e, xi, A, B, K, hold_policy=1, first=1):
    """One evaluation of the policy at hold step k.  e (nx) = x_meas - z_k; xi (N+1,nx) the column states (rows >= k are not read); A (N,nx,nx),
    B (N,nx,nu), K (N,N+1,nu,nx).  Returns (d, xi_new): d (nu) the input on top of the nominal v_k, xi_new with rows first..k-1 predicted and row k
    set.  hold_policy = 0 (the instance has no valid plan): d = 0 and xi unchanged."""
    xi = np.array(xi, dtype=float)
    nu = B.shape[2]
    if not hold_policy:
        return np.zeros(nu), xi
    assert first <= k < K.shape[0], (first, k, K.shape)
    new = xi.copy()
    acc = np.zeros(xi.shape[1])
    for j in range(first, k):
        new[j] = A[k - 1] @ xi[j] + B[k - 1] @ (K[k - 1, j] @ xi[j])
        acc = acc + new[j]
    new[k] = np.asarray(e, dtype=float) - acc
    d = np.zeros(nu)
    for j in range(first, k + 1):
        d = d + K[k, j] @ new[j]
    return d, new


def hold_step(model_id, k, x_meas, z_k, v_k, xi, A, B, K, E=None, w=None, hold_policy=1, plant=None):
    """A whole hold step of one instance: the policy on e = x_meas - z_k, then the plant (oracle/dyn_oracle.py's RK4 map unless `plant(x, u)` is
    given) and the noise E w.  Returns (u, x_next, xi_new)."""
    from oracle import dyn_oracle as DO
    x_meas = np.asarray(x_meas, dtype=float)
    d, new = policy(k, x_meas - np.asarray(z_k, dtype=float), xi, A, B, K, hold_policy=hold_policy)
    u = np.asarray(v_k, dtype=float) + d
    xp = np.asarray(plant(x_meas, u) if plant is not None else DO.ddyn(model_id, x_meas, u), dtype=float)
    if w is not None:
        xp = xp + np.asarray(E, dtype=float) @ np.asarray(w, dtype=float)
    return u, xp, new

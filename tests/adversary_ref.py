"""The state-feedback disturbance adversary (slsqp_cl_set_adversary) stated in numpy, independent of csrc/cl_adversary.hpp: which sample the plant step
of an instance at MPC step s reads, given its measured state.  The device kernels and the header's host build are compared with this bit for bit.

    direction d_i of state i
      policy 1 (nearest bound)     +1 when hi_i - x_i <= x_i - lo_i, else -1; a side that is +inf or >= 1e20 in the [hi; -lo] row is absent: only the
                                   other one pulls; neither: 0
      policy 2 (away from target)  +1 when x_i >= xref_i, else -1
      a NaN x_i: 0
    channel j: s_j = sum_i d_i E_ij (i ascending, additions of +-E_ij);  w_j = amp sign(s_j) where mask_j and s_j != 0, else the given W_j
"""
import numpy as np

OFF, NEAREST_BOUND, AWAY_FROM_TARGET = 0, 1, 2


def table_row(rows, b, s):
    """Row min(s, T - 1) of a table over MPC time: rows (T, W) shared by the batch or (B, T, W) per instance."""
    rows = np.asarray(rows, dtype=float)
    tab = rows[b] if rows.ndim == 3 else rows
    return tab[min(int(s), tab.shape[0] - 1)]


def directions(policy, x, g_row=None, xref=None):
    """d (nx,) in {-1, 0, +1}.  g_row: the stage row [hi; -lo] over [x; u] in force (policy 1); xref (nx,) or None = zero (policy 2)."""
    x = np.asarray(x, dtype=float)
    nx = len(x)
    d = np.zeros(nx, dtype=int)
    for i in range(nx):
        if np.isnan(x[i]):
            continue
        if policy == NEAREST_BOUND:
            nz = len(g_row) // 2
            hi, nlo = float(g_row[i]), float(g_row[nz + i])
            no_hi, no_lo = not (hi < 1e20), not (nlo < 1e20)
            if no_hi and no_lo:
                d[i] = 0
            elif no_lo:
                d[i] = 1
            elif no_hi:
                d[i] = -1
            else:
                d[i] = 1 if (hi - x[i]) <= (x[i] - (-nlo)) else -1
        elif policy == AWAY_FROM_TARGET:
            r = 0.0 if xref is None else float(xref[i])
            d[i] = 1 if x[i] >= r else -1
    return d


def applied(policy, amp, mask, x, E, W=None, g_row=None, xref=None):
    """w_applied (nx,) of one instance.  E (nx, nx) with its padded columns zero; W (nx,) the given sample or None (zeros); mask (nx,) or None (all)."""
    x = np.asarray(x, dtype=float)
    nx = len(x)
    E = np.asarray(E, dtype=float)
    Wv = np.zeros(nx) if W is None else np.asarray(W, dtype=float)
    if policy == OFF:
        return Wv.copy()
    d = directions(policy, x, g_row, xref)
    out = np.empty(nx)
    for j in range(nx):
        s = 0.0
        for i in range(nx):      # plain additions, i ascending
            if d[i] > 0:
                s = s + E[i, j]
            elif d[i] < 0:
                s = s - E[i, j]
        on = True if mask is None else bool(mask[j])
        out[j] = amp if (on and s > 0.0) else -amp if (on and s < 0.0) else Wv[j]
    return out


def applied_batch(policy, amp, mask, X, E, W=None, s=0, g=None, bounds=None, Xref=None):
    """w_applied (B, nx) for the measured states X (B, nx) of MPC step s.  g: the model's stage row; bounds: slsqp_cl_set_bounds' g table (T, ni) or
    (B, T, ni), overriding it; Xref: the reference's state table (T, nx) or (B, T, nx), or None."""
    X = np.asarray(X, dtype=float)
    out = np.empty_like(X)
    for b in range(X.shape[0]):
        g_row = table_row(bounds, b, s) if bounds is not None else g
        xr = None if Xref is None else table_row(Xref, b, s)
        out[b] = applied(policy, amp, mask, X[b], E, None if W is None else np.asarray(W)[b], g_row, xr)
    return out

"""Box bounds over MPC time for the on-device closed loops (slsqp_cl_set_bounds, include/slsqp.h): packing and checking of the rows, and the margin
of a closed-loop trajectory against them.  Plain numpy: needs no handle and no GPU.

Rows are in the model's own layout, G = [I; -I]: g (T, ni) = [hi; -lo] over [x; u], gf (T, ni_f) = [hi; -lo] over x; with a leading batch axis they
are per instance.  Row t belongs to MPC time t counted from the reset that starts a run; the last row is held."""
import numpy as np


def _check_rows(what, a, half):
    if np.isnan(a).any() or np.isneginf(a).any():
        raise ValueError(f"{what}: a NaN or -inf entry (+inf is \"no bound\")")
    if (a[..., :half] + a[..., half:] < 0.0).any():
        raise ValueError(f"{what}: a row with an upper bound below its lower bound")


def pack_bounds(model, g, gf=None, batch=None):
    """g (T,ni) or (B,T,ni), gf (T,ni_f) / (B,T,ni_f) or None (the model's own gf, repeated) -> (g, gf) as contiguous float64 arrays of matching
    rank, checked as the library checks them (shapes; no NaN or -inf; hi >= lo in every component).  batch: B of the handle, checked for per-instance
    rows."""
    ni, nif = int(model.ni), int(model.ni_f)
    g = np.ascontiguousarray(g, dtype=np.float64)
    if g.ndim not in (2, 3) or g.shape[-1] != ni or g.shape[-2] < 1:
        raise ValueError(f"bounds: g must be (T,{ni}) or (B,T,{ni}) with T >= 1, got {g.shape}")
    if g.ndim == 3 and batch is not None and g.shape[0] != int(batch):
        raise ValueError(f"bounds: per-instance rows need {int(batch)} leading rows, got {g.shape[0]}")
    if gf is None:
        gf = np.broadcast_to(np.asarray(model.gf, dtype=np.float64).ravel(), g.shape[:-1] + (nif,))
    gf = np.ascontiguousarray(gf, dtype=np.float64)
    if gf.shape != g.shape[:-1] + (nif,):
        raise ValueError(f"bounds: gf must be {g.shape[:-1] + (nif,)}, got {gf.shape}")
    _check_rows("bounds: g", g, ni // 2)
    _check_rows("bounds: gf", gf, nif // 2)
    return g, gf


def box_bounds(model, T, spec, batch=None):
    """Rows from per-component limits.  spec: {index into [x; u]: (lo, hi)}, each side a scalar, (T,), (B,T), or None for the model's own; every
    result is intersected with the model's box (a spec can only tighten it).  The terminal rows come from the state entries.  Returns (g, gf) of
    shape (T,·), or (B,T,·) as soon as one side is per instance (B = batch)."""
    nx, nz = int(model.nx), int(model.nx) + int(model.nu)
    T = int(T)
    if T < 1:
        raise ValueError("box_bounds: T must be >= 1")
    g0 = np.asarray(model.g, dtype=np.float64).ravel()
    per_inst = False
    sides = {}
    for idx, pair in spec.items():
        i = int(idx)
        if not 0 <= i < nz:
            raise ValueError(f"box_bounds: index {idx} outside [x; u] (0..{nz - 1})")
        if not (isinstance(pair, (tuple, list)) and len(pair) == 2):
            raise ValueError(f"box_bounds: entry {idx} must be a pair (lo, hi)")
        row = []
        for v in pair:
            if v is not None:
                v = np.asarray(v, dtype=np.float64)
                if v.ndim == 2:
                    if batch is None or v.shape != (int(batch), T):
                        raise ValueError(f"box_bounds: a per-instance side of entry {idx} must be ({batch},{T}), got {v.shape}")
                    per_inst = True
                elif v.ndim == 1 and v.shape != (T,):
                    raise ValueError(f"box_bounds: a time-varying side of entry {idx} must be ({T},), got {v.shape}")
                elif v.ndim > 2:
                    raise ValueError(f"box_bounds: a side of entry {idx} has {v.ndim} axes")
            row.append(v)
        sides[i] = row
    lead = (int(batch), T) if per_inst else (T,)
    g = np.broadcast_to(g0, lead + (2 * nz,)).copy()
    for i, (lo, hi) in sides.items():
        if hi is not None:
            g[..., i] = np.minimum(g[..., i], np.broadcast_to(hi, lead))
        if lo is not None:
            g[..., nz + i] = np.minimum(g[..., nz + i], -np.broadcast_to(lo, lead))      # -lo: a larger lo is a smaller entry
    gf0 = np.asarray(model.gf, dtype=np.float64).ravel()
    gf = np.concatenate([np.minimum(g[..., :nx], gf0[:nx]), np.minimum(g[..., nz:nz + nx], gf0[nx:])], axis=-1)
    return pack_bounds(model, g, gf, batch)


def bounds_window(g, gf, s, N):
    """The rows of MPC step s of ONE instance: g (T,ni), gf (T,ni_f) -> (g_win (N,ni), gf_row (ni_f,)), stage k the row min(s + k, T - 1), the terminal
    stage min(s + N, T - 1)."""
    T = g.shape[0]
    return g[np.minimum(s + np.arange(N), T - 1)], gf[min(s + N, T - 1)]


def constraint_margin(model, g, state_trajectory, input_trajectory):
    """state_trajectory (B,nx,steps), input_trajectory (B,nu,steps-1 or steps) of a closed-loop run, g (T,ni) or (B,T,ni): (steps, B), the smallest
    g_row(t)[i] - (G [x_meas(t); u0(t)])[i] over the finite rows of MPC time t (row min(t, T - 1)); negative: the true closed loop left the box in
    force at that time.  Where the run holds no input for a step (the last one of the reference's layout) only the state rows count."""
    x = np.asarray(state_trajectory, dtype=np.float64)
    u = np.asarray(input_trajectory, dtype=np.float64)
    B, nx, steps = x.shape
    nu = u.shape[1]
    nz = nx + nu
    g = np.asarray(g, dtype=np.float64)
    if g.ndim == 2:
        g = np.broadcast_to(g, (B,) + g.shape)
    out = np.full((steps, B), np.inf)
    for t in range(steps):
        r = g[:, min(t, g.shape[1] - 1)]                         # (B, ni)
        z = np.full((B, nz), np.nan)
        z[:, :nx] = x[:, :, t]
        if t < u.shape[2]:
            z[:, nx:] = u[:, :, t]
        m = np.concatenate([r[:, :nz] - z, r[:, nz:] + z], axis=1)
        m = np.where(np.isfinite(r) & ~np.isnan(m), m, np.inf)
        out[t] = m.min(axis=1)
    return out

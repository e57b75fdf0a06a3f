"""The measurement-noise rule of the closed loops in numpy (slsqp_cl_set_meas_noise, csrc/cl_meas.hpp): the controller of
instance b sees x_meas = x_plant + n_s at MPC step s, n_s row min(s, T - 1) of a table (T,nx) shared by the batch or (B,T,nx) per instance.  One
fp64 addition per component, so these are the device's bits."""
import numpy as np


def row_index(s, T):
    """The table's row for MPC step s: the last one is held."""
    return min(max(int(s), 0), int(T) - 1)


def rows(table, B, s):
    """(B,nx): the row of every instance for MPC step s."""
    table = np.asarray(table, dtype=float)
    r = table[..., row_index(s, table.shape[-2]), :]
    return np.broadcast_to(r, (B, table.shape[-1])).copy()


def measure(x_plant, table, s):
    """(B,nx): what the controllers see at step s when the true states are x_plant (B,nx)."""
    x_plant = np.asarray(x_plant, dtype=float)
    return x_plant + rows(table, x_plant.shape[0], s)


def measured_trajectory(state_trajectory, table):
    """(B,nx,steps) from the true trajectory (B,nx,steps)."""
    X = np.asarray(state_trajectory, dtype=float)
    return np.stack([measure(X[:, :, s], table, s) for s in range(X.shape[2])], axis=2)


def simulate(table, x0, deltas, S):
    """The two halves of the rule around a stand-in plant step x <- x + deltas[s] (deltas (steps,B,nx)), from slsqp_cl_init's x_plant <- x0,
    x_meas <- x0 + n_0.  Returns x_plant, x_meas after the last step and the logs (B,S,nx) of the truth and of the measurement at the top of every
    step (entries past the log's end are not written; unwritten entries stay -777)."""
    x0 = np.asarray(x0, dtype=float)
    B, nx = x0.shape
    xp, xm = x0.copy(), measure(x0, table, 0)
    lg_p, lg_m = np.full((B, S, nx), -777.0), np.full((B, S, nx), -777.0)
    for s, d in enumerate(np.asarray(deltas, dtype=float)):
        if s < S:
            lg_p[:, s], lg_m[:, s] = xp, xm
        xp = xp + d
        xm = measure(xp, table, s + 1)
    return xp, xm, lg_p, lg_m

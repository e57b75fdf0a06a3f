#!/usr/bin/env python3
"""Golden fixtures for the plant parameters: the reference's OWN ode / ddyn of the quadrotor and the rocket after changed values were written into
`model.params` (dyn/quadrotor.py:32-40, dyn/rocket.py:25-39).  Runs only where the reference is checked out; tests read only the .npz files.

Same approach as gen_golden.py (whose stubs and model set-up are imported, not edited): the reference's source is imported and evaluated through the
NumPy stand-in for the casadi functions its ODEs call; nothing of it is copied.

Per plant three parameter sets; every parameter is changed in at least one set, each by a different factor in 0.7 .. 1.4, the gimbal lengths by at
most 2 % (the linkage has no real solution far from its design values).  Evaluated at the points of dyn_{plant}_script.npz, which include the
saturated-actuator points.  Writes dyn_quadrotor_params.npz and dyn_rocket_params.npz with
    P (3, np)   X (npts, nx)   U (npts, nu)   ode (3, npts, nx)   ddyn (3, npts, nx)
The pendulum of the reference keeps its constants local to `ode`: no fixture (tests/plant_params_helpers.py carries a numpy statement instead).
"""
import os

import numpy as np

import gen_golden as G

OUT = os.path.dirname(os.path.abspath(__file__))

# factor per (set, parameter); 1.0 = unchanged.  All factors other than 1.0 differ from each other within a plant.
FACTORS = {
    "quadrotor": [  # m, g, l, Jx, Jy, Jz, kM
        [1.15, 1.0, 0.85, 1.30, 1.0, 0.75, 1.0],
        [1.0, 0.97, 1.0, 0.80, 1.25, 1.0, 1.40],
        [0.90, 1.03, 1.10, 1.0, 0.70, 1.20, 0.72],
    ],
    "rocket": [  # mass, gravity, Jxx, Jyy, Jzz, cog offset, tau_thrust, tau_servo, gimbal a, b, c, d, e
        [1.15, 1.0, 1.30, 0.80, 1.0, 1.10, 1.0, 1.35, 1.01, 1.0, 0.99, 1.0, 1.005],
        [0.85, 1.02, 1.0, 1.25, 0.75, 1.0, 1.40, 1.0, 1.0, 1.004, 1.0, 0.985, 1.0],
        [1.05, 0.97, 0.70, 1.0, 1.20, 0.90, 0.72, 0.78, 0.98, 0.996, 1.008, 1.015, 0.992],
    ],
}


def main():
    G.install_stubs()
    for name in ("quadrotor", "rocket"):
        m = G.model_setup(name)[0]
        keys = list(m.params.keys())
        dflt = np.array([m.params[k] for k in keys], dtype=float)
        F = np.array(FACTORS[name], dtype=float)
        assert F.shape == (3, len(keys))
        assert np.all((F != 1.0).any(axis=0)), "every parameter changes in at least one set"
        ch = F[F != 1.0]
        assert len(set(ch.tolist())) == len(ch) and ch.min() >= 0.7 and ch.max() <= 1.4
        if name == "rocket":
            assert F[:, 8:].min() >= 0.98 and F[:, 8:].max() <= 1.02
        pts = np.load(os.path.join(OUT, f"dyn_{name}_script.npz"))
        X, U = pts["X"], pts["U"]
        P = F * dflt[None, :]
        ode = np.zeros((3,) + X.shape)
        ddyn = np.zeros((3,) + X.shape)
        for s in range(3):
            for k, v in zip(keys, P[s]):
                m.params[k] = float(v)
            for i in range(X.shape[0]):
                ode[s, i] = np.asarray(m.ode(X[i], U[i]), dtype=float).reshape(-1)
                ddyn[s, i] = np.asarray(m.ddyn(X[i], U[i]), dtype=float).reshape(-1)
        assert np.all(np.isfinite(ode)) and np.all(np.isfinite(ddyn)), "a fixture value is NaN"
        assert np.abs(ddyn - pts["ddyn"][None]).max() > 1e-6      # the parameters reach the values
        np.savez_compressed(os.path.join(OUT, f"dyn_{name}_params.npz"), P=P, X=X, U=U, ode=ode, ddyn=ddyn, names=np.array(keys))
        print("wrote", name, P.shape, X.shape, "max |ddyn_p - ddyn|", float(np.abs(ddyn - pts["ddyn"][None]).max()))


if __name__ == "__main__":
    main()

"""Every closed-loop route in every state of the per-handle options (reference, plant parameters, bounds on or off) at the smallest shape, all logs
and final arrays into ONE .npz: run once per library (SLSQP_SO names another build) and compare the two files, which must be identical bit for bit
when a change claims to leave the arithmetic alone.

    python scripts/option_state_bits.py OUT.npz            # the runs of tests/loop_args_runs.py::option_state_runs, pendulum N = 3, B = 5, 3 steps
    python scripts/option_state_bits.py A.npz B.npz        # compare: prints every array that differs, exit status 1 if any does
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def record(path):
    import loop_args_runs as R
    from robust_nonlinear_mpc_amd import _lib
    arrays = {}
    for state in R.STATES:
        tag = "".join(map(str, state))
        m, N, B, steps, x0, W, kw = R.setup("pendulum")
        cl = R.make(m, N, B, **R.option_state(m, B, state))      # slsqp_nominal_solve alone
        cl.reset(x0, **kw)
        for k, v in R.final(cl).items():
            arrays[f"{tag}/nominal_solve/{k}"] = v
        cl.close()
        for route, (out, fin) in R.option_state_runs(state).items():
            assert R.real_work(out), (tag, route)
            for k in R.LOG_KEYS:
                arrays[f"{tag}/{route}/{k}"] = out[k]
            for k in R.FIN_KEYS:
                arrays[f"{tag}/{route}/fin/{k}"] = fin[k]
    np.savez(path, **arrays)
    print("option_state_bits:", len(arrays), "arrays from", _lib.SO_PATH, "->", path)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files)) + [k for k in A.files if k in B.files and not np.array_equal(A[k], B[k], equal_nan=True)]
    for k in bad:
        print("differs:", k)
    print("option_state_bits:", len(A.files), "arrays,", len(bad), "differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[1:3]) if len(sys.argv) > 2 else record(sys.argv[1]))

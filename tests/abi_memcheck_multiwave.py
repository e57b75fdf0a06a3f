"""Run by tests/test_gpu_multiwave.py::test_new_entry_points_under_debug_allocators in a child process with MALLOC_CHECK_=3 and
PYTHONMALLOC=malloc_debug (see tests/abi_memcheck.py): the entry points of the multi-wave path that take host buffers, once each, with buffers of
exactly the documented sizes -- slsqp_ne_solve writes W (B, N nx), G (B, n), bmax (B) and fail (B ints)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C
import numpy as np
from robust_nonlinear_mpc_amd import BatchedFastSLS, make_batch
GOLDEN = os.path.join(ROOT, "tests", "golden")

batch = make_batch("pendulum", os.path.join(GOLDEN, "sweep_pendulum_N10_s0.npz"), 3, seed=1)
m, N = batch["model"], batch["N"]
f = BatchedFastSLS(N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=3)
f.update_dynamics_list(batch["A"], batch["B"], batch["E"], batch["g"], batch["gN"], batch["c"])
f.update_linear_cost(batch["q"])
rng = np.random.default_rng(0)
PI, V = rng.uniform(0.1, 1.0, (3, f.n)), rng.normal(size=(3, f.n))
for waves in (1, 2, 8):
    out = f.ne_solve(PI, V, waves=waves)
    out2 = f.ne_solve(PI, V, waves=waves, factor=False)
    assert out["nu"].shape == (3, N, m.nx) and np.isfinite(out["nu"]).all() and np.isfinite(out2["G"]).all() and (out["fail"] == 0).all()
# the optional outputs may be NULL
W, G = np.empty((3, N * m.nx)), np.empty((3, f.n))
assert f.lib.slsqp_ne_solve(f.h, 4, 1, PI.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p), 1e-13, W.ctypes.data_as(C.c_void_p), G.ctypes.data_as(C.c_void_p), None, None, 0) == 0
assert f.lib.slsqp_ne_solve(f.h, 4, 1, None, V.ctypes.data_as(C.c_void_p), 1e-13, W.ctypes.data_as(C.c_void_p), G.ctypes.data_as(C.c_void_p), None, None, 0) != 0
f.opts.solve_waves = 4
assert f.opts.solve_waves == 4 and f.lib.slsqp_get_solve_waves(f.h) == 4
out = f.solve(batch["x0_arg"])
assert out["success"].all()
f.opts.solve_waves = 1
f.close()
print("abi_memcheck_multiwave ok")

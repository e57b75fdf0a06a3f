"""Run by tests/test_gpu_reference.py::test_setter_under_debug_allocators in a child process with MALLOC_CHECK_=3 and PYTHONMALLOC=malloc_debug (see
tests/abi_memcheck.py): slsqp_cl_set_reference with host buffers of exactly the documented sizes -- Xref (T,nx), Uref (T,nu) shared, (B,T,nx),
(B,T,nu) per instance, Uref NULL, T = 1 -- each followed by a closed-loop step that reads the reference, then cleared."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C
import numpy as np
from robust_nonlinear_mpc_amd import ClosedLoopMPC, get_model
from robust_nonlinear_mpc_amd import _lib as L

m = get_model("pendulum")
N, B = 10, 3
cl = ClosedLoopMPC(m, N, B)
lib, h = cl.f.lib, cl.f.h
x0 = np.tile(m.extra["x0"], (B, 1))
rng = np.random.default_rng(0)
ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
for T, per in ((1, 0), (5, 0), (1, 1), (N + 7, 1)):
    lead = (B,) if per else ()
    Xref = np.ascontiguousarray(0.3 * rng.uniform(-1, 1, lead + (T, m.nx)))
    Uref = np.ascontiguousarray(0.3 * rng.uniform(-1, 1, lead + (T, m.nu)))
    for U in (Uref, None):
        L.check(lib.slsqp_cl_set_reference(h, ptr(Xref), ptr(U), T, per, L.HOST))
        cl.reset(x0)
        r = cl.step(None)
        assert np.isfinite(r["nominal_x"]).all() and r["success"].any()
assert lib.slsqp_cl_set_reference(h, ptr(Xref), None, -1, 0, L.HOST) != 0
L.check(lib.slsqp_cl_set_reference(h, None, None, 0, 0, L.HOST))
cl.reset(x0)
assert cl.step(None)["success"].all()
cl.close()
print("abi_memcheck_reference ok")

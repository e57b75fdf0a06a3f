"""Host-side pieces of the persistent SCP closed loop (slsqp_cl_run_scp): the C declaration and its ctypes mirror, the unchanged option struct, and
the predicate that routes Monte-Carlo slices to the persistent launch.  No GPU needed."""
import ctypes
import os
import re

from conftest import ROOT


def _declaration(name):
    src = open(os.path.join(ROOT, "include", "slsqp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert mt, f"{name} is not declared in include/slsqp.h"
    return [a.strip() for a in mt.group(1).split(",")]


def test_header_declares_slsqp_cl_run_scp_and_the_loader_binds_it():
    import inspect
    from robust_nonlinear_mpc_amd import _lib
    args = _declaration("slsqp_cl_run_scp")
    assert len(args) == 6 and args[0].startswith("slsqp_handle") and args[1] == "int steps" and args[2] == "int rti" and "slsqp_opts" in args[5]
    assert len(_declaration("slsqp_cl_run")) == 8          # the existing entry point keeps its signature
    assert "slsqp_cl_run_scp" in _lib.EXPORTS
    mt = re.search(r"lib\.slsqp_cl_run_scp\.argtypes\s*=\s*\[([^\]]*)\]", inspect.getsource(_lib.load))
    assert mt and len(mt.group(1).split(",")) == len(args)


def test_option_struct_is_unchanged():
    from robust_nonlinear_mpc_amd import _lib
    assert ctypes.sizeof(_lib.Opts) == 104          # the parent commit's value: no new field, every caller's struct stays valid
    assert [f[0] for f in _lib.Opts._fields_][-2:] == ["fuse_rti", "cl_persistent"]


def test_can_run_persistent():
    from robust_nonlinear_mpc_amd import _lib, can_run_persistent
    env = {}
    assert can_run_persistent(1, 1, environ=env) and can_run_persistent(3, 2, environ=env) and can_run_persistent(-1, 2, environ=env)
    assert not can_run_persistent(3, None, environ=env) and not can_run_persistent(3, 0, environ=env)
    o = _lib.Opts()
    o.fuse_rti, o.precision = 1, 0
    assert can_run_persistent(3, 2, o, environ=env)
    o.precision = 1
    assert not can_run_persistent(3, 2, o, environ=env)
    o.precision, o.fuse_rti = 0, 0
    assert not can_run_persistent(3, 2, o, environ=env)
    assert not can_run_persistent(3, 2, environ={"SLSQP_FUSE_RTI": "0"})
    assert not can_run_persistent(1, 1, environ={"SLSQP_SWEEP_SHARED": "0"})
    assert can_run_persistent(3, 2, environ={"SLSQP_FUSE_RTI": "1"})

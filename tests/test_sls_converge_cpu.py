"""Host-side pieces of fast-SLS converge mode inside the persistent closed loop (slsqp_cl_set_sls_converge): the C declarations and their ctypes
mirror, the predicate that routes Monte-Carlo slices to the persistent launch, and tests/cl_sls_conv_check_main.cpp, a stand-alone program with its
own main around csrc/cl_sls_conv.hpp's rule and csrc/slsqp_api.hip's option and argument builders (compiled for the host only), built with the address
and undefined-behaviour sanitizers.  No GPU needed."""
import inspect
import os
import re
import subprocess

from conftest import ROOT


def _declaration(name):
    src = open(os.path.join(ROOT, "include", "slsqp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert mt, f"{name} is not declared in include/slsqp.h"
    return [a.strip() for a in mt.group(1).split(",")]


def test_header_declares_the_two_entry_points_and_the_loader_binds_them():
    from robust_nonlinear_mpc_amd import _lib
    args = _declaration("slsqp_cl_set_sls_converge")
    assert len(args) == 2 and args[0].startswith("slsqp_handle") and args[1] == "int on"
    args = _declaration("slsqp_cl_get_sls_converge")
    assert len(args) == 1 and args[0].startswith("slsqp_handle")
    assert len(_declaration("slsqp_cl_run_scp")) == 6          # the entry point that reads the option keeps its signature
    src = inspect.getsource(_lib.load)
    for name, n in (("slsqp_cl_set_sls_converge", 2), ("slsqp_cl_get_sls_converge", 1)):
        assert name in _lib.EXPORTS
        mt = re.search(r"lib\." + name + r"\.argtypes\s*=\s*\[([^\]]*)\]", src)
        assert mt and len(mt.group(1).split(",")) == n
    api = open(os.path.join(ROOT, "robust-nonlinear-mpc_amd", "csrc", "slsqp_api.hip")).read()
    for name in ("slsqp_cl_set_sls_converge", "slsqp_cl_get_sls_converge"):
        assert re.search(r'extern "C" int ' + name + r"\(", api)


def test_can_run_persistent_with_and_without_the_keyword():
    from robust_nonlinear_mpc_amd import _lib, can_run_persistent
    env = {}
    # the default keeps every answer
    assert not can_run_persistent(3, None, environ=env) and not can_run_persistent(3, 0, environ=env) and not can_run_persistent(-1, -2, environ=env)
    assert not can_run_persistent(3, None, environ=env, sls_converge=False)
    assert can_run_persistent(3, 2, environ=env) and can_run_persistent(3, 2, environ=env, sls_converge=True)
    # the keyword admits fast-SLS converge mode, for every rti
    for rti in (1, 2, 3, -1, 0):
        for k in (None, 0, -1):
            assert can_run_persistent(rti, k, environ=env, sls_converge=True)
    # ... and nothing else the loop refuses
    o = _lib.Opts()
    o.fuse_rti, o.precision, o.max_sls_iter = 1, 0, 30
    assert can_run_persistent(2, None, o, environ=env, sls_converge=True) and not can_run_persistent(2, None, o, environ=env)
    o.max_sls_iter = 0
    assert not can_run_persistent(2, None, o, environ=env, sls_converge=True) and can_run_persistent(2, 2, o, environ=env, sls_converge=True)
    o.max_sls_iter, o.precision = 30, 1
    assert not can_run_persistent(2, None, o, environ=env, sls_converge=True)
    o.precision, o.fuse_rti = 0, 0
    assert not can_run_persistent(2, None, o, environ=env, sls_converge=True)
    assert not can_run_persistent(2, None, environ={"SLSQP_FUSE_RTI": "0"}, sls_converge=True)
    assert not can_run_persistent(2, None, environ={"SLSQP_SWEEP_SHARED": "0"}, sls_converge=True)
    assert not can_run_persistent(2, None, environ={"SLSQP_PRECISION": "1"}, sls_converge=True)


def test_python_layers_take_the_option():
    """The keyword reaches run_decoupled, run_monte_carlo and the slice runner, off by default everywhere."""
    from robust_nonlinear_mpc_amd import BatchedFastSLS, ClosedLoopMPC, run_monte_carlo
    from robust_nonlinear_mpc_amd.monte_carlo import _run_slice
    for fn in (ClosedLoopMPC.run_decoupled, run_monte_carlo, _run_slice):
        p = inspect.signature(fn).parameters
        assert "persistent_converge" in p and p["persistent_converge"].default is False
    assert hasattr(BatchedFastSLS, "set_sls_converge") and hasattr(BatchedFastSLS, "get_sls_converge")


def test_rule_option_and_block_layout_under_sanitizers():
    """The "took no part" rule of cl_sls_conv.hpp against a brute-force model of the batch-wide launches on every table of iteration counts for caps
    1..4 and up to 4 instances; slsqp_cl_set_sls_converge's range with refusals that change nothing and slsqp_cl_run_scp's answer to rti_steps with
    the option off and on; cl_options with the var values of the option off in all 16 states; ScpLoopArgs with the size and field offsets it had,
    the hold and plan blocks where they were and the new block behind them; a staged block that does not depend on the option."""
    exe = os.path.join(ROOT, "tests", "_build", "cl_sls_conv_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-fuse-cuid=none", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Wno-pass-failed",
                           "-Wno-invalid-offsetof", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cl_sls_conv_check_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cl_sls_conv_check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

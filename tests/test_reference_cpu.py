"""Reference tracking, the part that needs no GPU: the C ABI declares and binds slsqp_cl_set_reference, slsqp_opts keeps its layout, and the CPU
restatement of the tracked closed loop (tests/reference_cases.py) is well posed for every case tests/test_gpu_reference.py holds the GPU against."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from reference_cases import case, oracle_case


def test_header_declares_the_setter_with_six_arguments_and_the_loader_binds_it():
    from robust_nonlinear_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "slsqp.h")).read()
    decl = re.search(r"\bint\s+slsqp_cl_set_reference\s*\(([^)]*)\)\s*;", header)
    assert decl, "slsqp_cl_set_reference is not declared in include/slsqp.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 6, args
    assert args[0].startswith("slsqp_handle") and args[1].startswith("const double") and args[2].startswith("const double")
    assert [a.split()[0] for a in args[3:]] == ["int", "int", "int"]
    assert "slsqp_cl_set_reference" in _lib.EXPORTS
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert len(lib.slsqp_cl_set_reference.argtypes) == 6


def test_opts_keep_their_layout():
    from robust_nonlinear_mpc_amd import _lib
    assert ctypes.sizeof(_lib.Opts) == 104
    header = open(os.path.join(ROOT, "include", "slsqp.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} slsqp_opts;", header, re.S).group(1)
    assert "ref" not in re.sub(r"/\*.*?\*/", "", body, flags=re.S)      # the reference is a property of the handle


@pytest.mark.parametrize("name,b", [(n, b) for n in ("A", "B") for b in range(3)])
def test_cpu_closed_loop_with_a_reference_is_well_posed(name, b):
    """Every step of the tracked CPU loop succeeds and every QP of the ADMM restatement converges: the GPU test may hold its results against these
    at 1e-6.  And the reference matters: the trajectory differs from the untracked one by far more than that."""
    c = case(name)
    ref = oracle_case(name, b)
    assert ref["success"].all(), ref["success"]
    assert ref["oracle_qp_converged"].all(), ref["oracle_qp_converged"]
    from problems import run_oracle_closed_loop
    m = c["m"]
    plain = run_oracle_closed_loop(m, c["N"], c["x0"][b], c["steps"], m.rti, m.fast_sls_rti_steps)
    diff = np.abs(ref["nominal_x"] - plain["nominal_x"]).max(axis=(1, 2))
    print(name, b, "tracked vs untracked, per step:", diff)
    assert diff.max() > 1e-4


@pytest.mark.parametrize("name", ["A", "B"])
def test_setpoint_of_one_row_equals_the_same_row_repeated(name):
    """T = 1 and T = steps + N + 1 equal rows: the last row is held, so the CPU trajectories are identical."""
    c = case(name)
    one, many = oracle_case(name, 0, 1), oracle_case(name, 0, c["steps"] + c["N"] + 1)
    for k in ("state", "u0", "nominal_x", "nominal_u", "success"):
        assert np.array_equal(one[k], many[k]), k

"""Time-varying box bounds, the part that needs no GPU: the setter's validation and packing routine in a stand-alone program built with the address
and undefined-behaviour sanitizers, pack_bounds / box_bounds / bounds_window / constraint_margin, the C ABI's declaration and its ctypes mirror, and
the CPU restatement of the bounded closed loop (tests/bounds_cases.py) for every case tests/test_gpu_bounds.py holds the GPU against."""
import os
import re
import subprocess

import numpy as np
import pytest

import bounds_cases as BC
from conftest import ROOT


def test_validation_routine_under_sanitizers():
    """csrc/cl_bounds.hpp (free of HIP calls) in a stand-alone program with its own main, built with -fsanitize=address,undefined: every refusal of
    slsqp_cl_set_bounds that depends on the values or the call's own arguments, +inf accepted, the shared and per-instance layouts, buffers of exactly
    the documented sizes."""
    exe = os.path.join(ROOT, "tests", "_build", "cl_bounds_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    # (the sanitizer runtimes linked statically: the program needs nothing from its environment)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-o", exe, os.path.join(ROOT, "tests", "cl_bounds_check_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cl_bounds_check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_header_declares_the_setter_and_the_loader_binds_it():
    from robust_nonlinear_mpc_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slsqp.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+slsqp_cl_set_bounds\s*\(([^)]*)\)\s*;", header)
    assert decl, "slsqp_cl_set_bounds is not declared in include/slsqp.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 6, args
    assert args[0].startswith("slsqp_handle") and args[1].startswith("const double") and args[2].startswith("const double")
    assert [a.split() for a in args[3:]] == [["int", "T"], ["int", "per_instance"], ["int", "loc"]]
    assert "slsqp_cl_set_bounds" in _lib.EXPORTS
    import ctypes
    assert ctypes.sizeof(_lib.Opts) == 104      # the bounds are a property of the handle
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert lib.slsqp_cl_set_bounds.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]


def test_pack_bounds():
    from robust_nonlinear_mpc_amd import get_model, pack_bounds
    m = get_model("pendulum")
    B, T = 3, 4
    g1 = np.tile(m.g, (T, 1))
    g, gf = pack_bounds(m, g1)
    assert g.shape == (T, m.ni) and gf.shape == (T, m.ni_f) and np.array_equal(gf, np.tile(m.gf, (T, 1))) and g.flags.c_contiguous and gf.flags.c_contiguous
    gB = np.tile(m.g, (B, T, 1))
    g, gf = pack_bounds(m, gB, batch=B)
    assert g.shape == (B, T, m.ni) and gf.shape == (B, T, m.ni_f)
    g, gf = pack_bounds(m, gB, 0.5 * np.tile(m.gf, (B, T, 1)), batch=B)
    assert np.array_equal(gf, 0.5 * np.tile(m.gf, (B, T, 1)))
    inf = g1.copy(); inf[1, 0] = np.inf; inf[1, m.nz] = np.inf
    assert np.isinf(pack_bounds(m, inf)[0][1, 0])
    for bad, word in ((np.tile(m.g, (B + 1, T, 1)), "leading"), (g1[:, :-1], "must be"), (np.zeros((0, m.ni)), "T >= 1"), (m.g, "must be")):
        with pytest.raises(ValueError, match=word):
            pack_bounds(m, bad, batch=B)
    with pytest.raises(ValueError, match="gf must be"):
        pack_bounds(m, g1, np.tile(m.gf, (T + 1, 1)))
    for v in (np.nan, -np.inf):
        b = g1.copy(); b[2, 3] = v
        with pytest.raises(ValueError, match="NaN or -inf"):
            pack_bounds(m, b)
        bf = np.tile(m.gf, (T, 1)); bf[0, 1] = v
        with pytest.raises(ValueError, match="NaN or -inf"):
            pack_bounds(m, g1, bf)
    b = g1.copy(); b[0, 1] = -b[0, m.nz + 1] - 1e-9
    with pytest.raises(ValueError, match="below"):
        pack_bounds(m, b)


def test_box_bounds():
    from robust_nonlinear_mpc_amd import box_bounds, get_model
    m = get_model("rocket")
    nx, nz, B, T = m.nx, m.nz, 3, 5
    g, gf = box_bounds(m, T, {})
    assert g.shape == (T, m.ni) and gf.shape == (T, m.ni_f) and np.array_equal(g, np.tile(m.g, (T, 1))) and np.array_equal(gf, np.tile(m.gf, (T, 1)))
    # a scalar upper side on an input, None for the lower: the model's own lower side stays
    iu = nx + 2
    g, gf = box_bounds(m, T, {iu: (None, 0.5 * m.u_ub[2])})
    assert np.all(g[:, iu] == 0.5 * m.u_ub[2]) and np.array_equal(g[:, nz + iu], np.tile(m.g[nz + iu], T)) and np.array_equal(gf, np.tile(m.gf, (T, 1)))
    # intersection: a side wider than the model's keeps the model's; a time-varying state side reaches the terminal rows
    lo_t = np.linspace(m.x_lb[1] - 1.0, 0.5 * m.x_lb[1], T)
    g, gf = box_bounds(m, T, {1: (lo_t, 10.0 * abs(m.x_ub[1]) + 1.0)})
    assert np.array_equal(g[:, 1], np.tile(m.x_ub[1], T))
    assert np.array_equal(g[:, nz + 1], np.minimum(-lo_t, -m.x_lb[1])) and g[0, nz + 1] == -m.x_lb[1] and g[-1, nz + 1] == -0.5 * m.x_lb[1]
    assert np.array_equal(gf[:, 1], g[:, 1]) and np.array_equal(gf[:, nx + 1], g[:, nz + 1])
    other = [i for i in range(m.ni) if i not in (1, nz + 1)]
    assert np.array_equal(g[:, other], np.tile(m.g[other], (T, 1)))
    # per instance as soon as one side is (B,T)
    hiB = np.tile(m.x_ub[0], (B, T)) * np.array([0.9, 0.8, 0.7])[:, None]
    g, gf = box_bounds(m, T, {0: (None, hiB), iu: (np.inf * -1, np.inf)}, batch=B)
    assert g.shape == (B, T, m.ni) and gf.shape == (B, T, m.ni_f) and np.array_equal(g[:, :, 0], hiB) and np.array_equal(gf[:, :, 0], hiB)
    assert np.array_equal(g[:, :, iu], np.full((B, T), m.u_ub[2])) and np.array_equal(g[:, :, nz + iu], np.full((B, T), -m.u_lb[2]))      # infinite sides: the model's
    for spec, word in (({nz: (0, 1)}, "outside"), ({-1: (0, 1)}, "outside"), ({0: 1.0}, "pair"), ({0: (np.zeros(T + 1), None)}, "time-varying"),
                       ({0: (None, np.zeros((B + 1, T)))}, "per-instance"), ({0: (np.zeros((2, 2, 2)), None)}, "axes")):
        with pytest.raises(ValueError, match=word):
            box_bounds(m, T, spec, batch=B)
    with pytest.raises(ValueError, match="per-instance"):
        box_bounds(m, T, {0: (None, np.zeros((B, T)))})      # (B,T) without batch
    with pytest.raises(ValueError, match="below"):
        box_bounds(m, T, {0: (m.x_ub[0] + 1.0, None)})       # lower side above the model's upper side
    with pytest.raises(ValueError, match="NaN"):
        box_bounds(m, T, {0: (None, np.nan)})
    with pytest.raises(ValueError, match="T must"):
        box_bounds(m, 0, {})


@pytest.mark.parametrize("T,s", [(1, 0), (1, 5), (4, 0), (4, 2), (9, 3), (12, 4), (30, 0)])
def test_bounds_window_against_a_hand_written_loop(T, s):
    """T = 1, T < N, T between s + 1 and s + N (the hold begins inside the horizon), T past the horizon; the package's and the test helper's."""
    from robust_nonlinear_mpc_amd import bounds_window
    N, ni, nif = 6, 10, 8
    rng = np.random.default_rng(T * 100 + s)
    g, gf = rng.uniform(1, 2, (T, ni)), rng.uniform(1, 2, (T, nif))
    want_g = np.zeros((N, ni))
    for k in range(N):
        t = s + k
        if t > T - 1:
            t = T - 1
        want_g[k] = g[t]
    tN = s + N if s + N <= T - 1 else T - 1
    for fn in (bounds_window, BC.bounds_window):
        gw, gfw = fn(g, gf, s, N)
        assert np.array_equal(gw, want_g) and np.array_equal(gfw, gf[tN])


def test_constraint_margin():
    from robust_nonlinear_mpc_amd import constraint_margin, get_model
    m = get_model("pendulum")
    nx, nz, B, steps = m.nx, m.nz, 2, 4
    g = np.tile(m.g, (3, 1)).astype(float)
    g[1:, 0] = 0.5                      # x_0 <= 0.5 from row 1 on (held past row 2)
    g[:, nx] = np.inf                   # no upper bound on the input at all
    x = np.zeros((B, nx, steps)); u = np.zeros((B, m.nu, steps - 1))
    x[0, 0] = [0.6, 0.4, 0.7, 0.45]; u[0, 0] = [1e9, 0.0, 0.0]
    cm = constraint_margin(m, g, x, u)
    assert cm.shape == (steps, B)
    z0 = np.concatenate([x[0, :, 0], u[0, :, 0]])
    rows0 = np.concatenate([m.g[:nz] - z0, m.g[nz:] + z0])
    assert cm[0, 0] == np.delete(rows0, nx).min() and rows0[nx] < 0      # row 0: the model's box, but the huge input is not held against its +inf row
    assert np.isclose(cm[1, 0], 0.1) and np.isclose(cm[2, 0], -0.2) and np.isclose(cm[3, 0], 0.05)      # row 3 = held row 2, state rows only (no input logged)
    assert np.all(cm[:, 1] > 0)
    gB = np.stack([g, np.tile(m.g, (3, 1))])
    assert np.array_equal(constraint_margin(m, gB, x, u)[:, 0], cm[:, 0])


@pytest.mark.parametrize("name", BC.CASES)
def test_cpu_closed_loop_with_bounds_is_well_posed(name):
    """Every step of the bounded CPU loop succeeds with a converged QP, the bounds matter (the closed-loop state differs from the unbounded loop's by
    more than 1e-3, so the GPU comparison at 1e-6 cannot pass with the bounds ignored), and the oracle's own trajectory stays inside the box in force
    (constraint_margin >= 0)."""
    from robust_nonlinear_mpc_amd import constraint_margin
    c = BC.case(name)
    m, steps = c["m"], c["steps"]
    ref, plain = BC.oracle_case(name), BC.oracle_case(name[0] + "0")
    assert ref["success"].all(), ref["success"]
    assert ref["oracle_qp_converged"].all(), ref["oracle_qp_converged"]
    assert plain["success"].all() and plain["oracle_qp_converged"].all()
    diff = np.abs(ref["state"] - plain["state"]).max()
    cm = constraint_margin(m, c["g"], ref["state"].T[None], ref["u0"][: steps - 1].T[None])
    print(name, "bounded vs unbounded closed-loop state:", diff, "smallest constraint_margin:", cm.min())
    assert diff > 1e-3
    assert cm.min() >= 0.0

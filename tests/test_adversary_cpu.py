"""The state-feedback disturbance adversary without a GPU (slsqp_cl_set_adversary): tests/cl_adversary_check_main.cpp, a
stand-alone program with its own main around csrc/cl_adversary.hpp's decision function and csrc/slsqp_api.hip's option and argument builders (compiled
for the host only), built with the address and undefined-behaviour sanitizers; a few hundred random cases through the same program's host shim against
tests/adversary_ref.py, bit for bit; the C declarations and their ctypes mirror; the Python argument handling."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import adversary_ref as AR
from conftest import ROOT

EXE = os.path.join(ROOT, "tests", "_build", "cl_adversary_check")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-fuse-cuid=none", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Wno-pass-failed",
                           "-Wno-invalid-offsetof", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", EXE,
                           os.path.join(ROOT, "tests", "cl_adversary_check_main.cpp")])
    return EXE


def test_rule_validation_options_and_block_layout_under_sanitizers(exe):
    """The table of cases of the decision function (tie, absent sides through +inf and 1e20, NaN state, a dense E whose sum cancels, a padded channel,
    mask, amp, policy 2 with and without a reference, row min(s, T - 1) of shared and per-instance tables, the log's last entry); the setter's
    validation; cl_options in the 16 option states with the adversary on; the argument block's layout."""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cl_adversary_check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _random_cases(n, seed):
    rng = np.random.default_rng(seed)
    cases = []
    for c in range(n):
        nx = int(rng.integers(1, 18))
        nu = int(rng.integers(1, 5))
        nz = nx + nu
        policy = int(rng.integers(0, 3))
        amp = float(rng.choice([0.5, 1.0, 1.5, rng.uniform(0.1, 2.0)]))
        mask = rng.integers(0, 2, nx) if rng.random() < 0.7 else np.ones(nx, dtype=int)
        lo = -rng.uniform(0.5, 3.0, nz)
        hi = rng.uniform(0.5, 3.0, nz)
        g = np.concatenate([hi, -lo])
        for i in range(nz):      # absent sides: +inf, 1e20, and above
            u = rng.random()
            if u < 0.12:
                g[i] = rng.choice([np.inf, 1e20, 5e20])
            if 0.08 < u < 0.2:
                g[nz + i] = rng.choice([np.inf, 1e20, 5e20])
        x = rng.uniform(-3.0, 3.0, nx)
        for i in range(nx):
            u = rng.random()
            if u < 0.1 and g[i] < 1e20 and g[nz + i] < 1e20:
                x[i] = 0.5 * (g[i] - g[nz + i])      # mid-box (a tie where the halves are exact)
            elif u < 0.15:
                x[i] = np.nan
            elif u < 0.2:
                x[i] = 0.0
        xref = np.where(rng.random(nx) < 0.3, x, rng.uniform(-1.0, 1.0, nx))      # x == xref: the >= side
        kind = rng.random()
        if kind < 0.4:
            E = np.diag(rng.uniform(-1.0, 1.0, nx))
        else:
            E = rng.integers(-4, 5, (nx, nx)) * 0.125      # exact sums: cancellations to zero happen
        nw = nx if rng.random() < 0.6 else int(rng.integers(1, nx + 1))
        E[:, nw:] = 0.0      # padded channels
        has_W = rng.random() < 0.8
        W = rng.uniform(-1.0, 1.0, nx)
        cases.append(dict(policy=policy, nx=nx, nz=nz, amp=amp, mask=mask, g=g, x=x, xref=xref, E=E, has_W=has_W, W=W))
    return cases


def test_host_build_of_the_header_equals_the_numpy_statement(exe, tmp_path):
    cases = _random_cases(400, 20240607)
    flat = []
    for c in cases:
        bits = int(sum(int(b) << j for j, b in enumerate(c["mask"])))
        flat += [float(c["policy"]), float(c["nx"]), float(c["nz"]), c["amp"], float(bits), 1.0 if c["has_W"] else 0.0]
        flat += list(c["x"]) + list(c["g"]) + list(c["xref"]) + list(c["E"].ravel()) + list(c["W"])
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    np.asarray(flat, dtype=np.float64).tofile(fin)
    r = subprocess.run([exe, "shim", fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    got = np.fromfile(fout, dtype=np.float64)
    assert got.size == sum(c["nx"] for c in cases)
    p, seen = 0, dict(pos=0, neg=0, kept=0, cancelled=0, tie=0)
    for c in cases:
        want = AR.applied(c["policy"], c["amp"], c["mask"], c["x"], c["E"], c["W"] if c["has_W"] else None, c["g"], c["xref"])
        w = got[p:p + c["nx"]]
        p += c["nx"]
        assert np.array_equal(w, want), c
        if c["policy"]:
            seen["pos"] += int(np.sum(w == c["amp"]))
            seen["neg"] += int(np.sum(w == -c["amp"]))
            given = c["W"] if c["has_W"] else np.zeros(c["nx"])
            seen["kept"] += int(np.sum((w == given) & (np.asarray(c["mask"]) == 0)))
            d = AR.directions(c["policy"], c["x"], c["g"], c["xref"])
            s = d @ c["E"]
            seen["cancelled"] += int(np.sum((s == 0) & (np.abs(d) @ np.abs(c["E"]) > 0)))
            if c["policy"] == AR.NEAREST_BOUND:
                seen["tie"] += int(np.sum((c["g"][:c["nx"]] - c["x"]) == (c["x"] + c["g"][c["nz"]:c["nz"] + c["nx"]])))
    assert all(v > 0 for v in seen.values()), seen      # every branch of the rule was taken


def test_reference_statement_on_known_cases():
    """adversary_ref itself, by hand: the diagonal reduction w_j = amp d_j sign(E_jj), the tie, the absent sides, the row that is held."""
    E = np.diag([0.5, -0.25, 0.0])
    g = np.array([2.0, 4.0, 1.0, 9.0, 2.0, 0.0, 1.0, 9.0])      # nx = 3, nu = 1
    w = AR.applied(AR.NEAREST_BOUND, 0.5, None, [0.0, 3.0, 0.1], E, [0.1, 0.2, 0.3], g)
    assert np.array_equal(w, [0.5, -0.5, 0.3])      # tie -> +1; pushed up through a negative E_jj; a zero column keeps the given sample
    g2 = g.copy()
    g2[0] = np.inf
    g2[5] = 1e20
    assert np.array_equal(AR.directions(AR.NEAREST_BOUND, [1.9, 0.1, np.nan], g2), [-1, 1, 0])
    assert np.array_equal(AR.directions(AR.AWAY_FROM_TARGET, [0.0, -0.1, 0.2], xref=[0.0, 0.0, 0.3]), [1, -1, -1])
    tab = np.arange(12.0).reshape(2, 3, 2)
    assert np.array_equal(AR.table_row(tab, 1, 7), [10.0, 11.0]) and np.array_equal(AR.table_row(tab[0], 1, 1), [2.0, 3.0])


def _declaration(name):
    src = open(os.path.join(ROOT, "include", "slsqp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert mt, f"{name} is not declared in include/slsqp.h"
    return [a.strip() for a in mt.group(1).split(",")]


def test_header_declares_the_entry_points_and_the_loader_binds_them():
    from robust_nonlinear_mpc_amd import _lib
    args = _declaration("slsqp_cl_set_adversary")
    assert len(args) == 4 and args[0].startswith("slsqp_handle") and args[1] == "int policy" and args[2] == "double amp" and args[3].startswith("const unsigned char *mask")
    args = _declaration("slsqp_cl_get_adversary")
    assert len(args) == 3 and args[1] == "int *policy" and args[2] == "double *amp"
    src = inspect.getsource(_lib.load)
    for name, n in (("slsqp_cl_set_adversary", 4), ("slsqp_cl_get_adversary", 3)):
        assert name in _lib.EXPORTS
        mt = re.search(r"lib\." + name + r"\.argtypes\s*=\s*\[([^\]]*)\]", src)
        assert mt and len(mt.group(1).split(",")) == n
    hdr = open(os.path.join(ROOT, "include", "slsqp.h")).read()
    from robust_nonlinear_mpc_amd.fast_sls import ADVERSARY_POLICIES
    for name, code in (("OFF", "off"), ("NEAREST_BOUND", "nearest_bound"), ("AWAY_FROM_TARGET", "away_from_target")):
        mt = re.search(r"#define SLSQP_ADV_" + name + r"\s+(\d+)", hdr)
        assert mt and int(mt.group(1)) == ADVERSARY_POLICIES[code] == getattr(AR, name)


def test_python_argument_handling_without_a_handle():
    from robust_nonlinear_mpc_amd import BatchedFastSLS, ClosedLoopMPC, run_monte_carlo
    from robust_nonlinear_mpc_amd.fast_sls import adversary_arguments
    from robust_nonlinear_mpc_amd.monte_carlo import _run_slice
    assert adversary_arguments(None) == (0, 1.0, None) and adversary_arguments("off", 0.3)[0] == 0 and adversary_arguments(0)[0] == 0
    assert adversary_arguments("nearest_bound", 0.5)[:2] == (1, 0.5) and adversary_arguments("away_from_target")[:2] == (2, 1.0)
    assert adversary_arguments(1)[0] == 1 and adversary_arguments(np.int64(2), 1.5)[:2] == (2, 1.5)
    assert adversary_arguments(None, float("nan"))[0] == 0      # clearing reads nothing else
    for bad in ("closest", 3, -1, 1.0, True, [1]):
        with pytest.raises(ValueError, match="unknown policy"):
            adversary_arguments(bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="amp must be finite and > 0"):
            adversary_arguments("nearest_bound", bad)
    code, amp, mk = adversary_arguments(2, 1.0, [1, 0, 2.5, 0], nx=4)
    assert mk.dtype == np.uint8 and mk.flags.c_contiguous and np.array_equal(mk, [1, 0, 1, 0])
    assert np.array_equal(adversary_arguments(1, 1.0, np.array([True, False]))[2], [1, 0])
    for bad, nx in (([1, 0], 4), ([[1, 0]], 2), (1, 1)):
        with pytest.raises(ValueError, match="mask must be"):
            adversary_arguments(1, 1.0, bad, nx=nx)
    # the keywords reach every layer, off by default
    for fn in (ClosedLoopMPC.__init__, run_monte_carlo, _run_slice):
        p = inspect.signature(fn).parameters
        assert p["adversary"].default is None and p["adversary_amp"].default == 1.0 and p["adversary_mask"].default is None
    assert hasattr(BatchedFastSLS, "set_adversary") and hasattr(BatchedFastSLS, "get_adversary") and hasattr(ClosedLoopMPC, "set_adversary")
    for ex in ("closed_loop.py", "rocket_closed_loop.py"):
        src = open(os.path.join(ROOT, "examples", ex)).read()
        assert '"--adversary"' in src and '"--adversary-amp"' in src

"""Measurement noise of the closed loops without a GPU (slsqp_cl_set_meas_noise): tests/cl_meas_noise_check_main.cpp, a
stand-alone program with its own main around csrc/cl_meas.hpp -- the row selection, the addition, the log write and the setter's validation --
built with the address and undefined-behaviour sanitizers; random tables through the same program's shim against tests/meas_noise_ref.py, bit for
bit; the C declaration and its ctypes mirror; the Python layers' argument handling and streams."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import meas_noise_ref as MR
from conftest import ROOT

EXE = os.path.join(ROOT, "tests", "_build", "cl_meas_noise_check")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-fuse-cuid=none", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Wno-pass-failed",
                           "-Wno-invalid-offsetof", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", EXE,
                           os.path.join(ROOT, "tests", "cl_meas_noise_check_main.cpp")])
    return EXE


def test_validation_rows_and_rule_under_sanitizers(exe):
    """Every refusal of the setter with a message that names its argument; row min(s, T - 1) on heap buffers of exactly (T,nx) and (B,T,nx); the two
    halves of the rule with a log of fewer entries than steps; the shared and the per-instance stride."""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cl_meas_noise_check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_host_build_of_the_header_equals_the_numpy_statement(exe, tmp_path):
    rng = np.random.default_rng(20240911)
    seen = dict(shared=0, per_instance=0, held=0, short_log=0, no_log=0, bias=0)
    for c in range(60):
        B, nx, T = int(rng.integers(1, 6)), int(rng.integers(1, 18)), int(rng.integers(1, 5))
        per, steps = int(rng.random() < 0.5), int(rng.integers(1, 7))
        S = int(rng.choice([0, max(steps - 2, 1), steps, steps + 2]))
        table = rng.uniform(-3e-3, 3e-3, ((B, T, nx) if per else (T, nx)))
        x0, d = rng.uniform(-2.0, 2.0, (B, nx)), rng.uniform(-0.1, 0.1, (steps, B, nx))
        fin, fout = str(tmp_path / f"c{c}.bin"), str(tmp_path / f"o{c}.bin")
        np.concatenate([[B, nx, T, per, S, steps], table.ravel(), x0.ravel(), d.ravel()]).astype(np.float64).tofile(fin)
        r = subprocess.run([exe, "shim", fin, fout], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        got = np.fromfile(fout, dtype=np.float64)
        xp, xm, lp, lm = MR.simulate(table, x0, d, S)
        want = np.concatenate([xp.ravel(), xm.ravel(), lp.ravel(), lm.ravel()])
        assert got.size == want.size and np.array_equal(got, want), (c, B, nx, T, per, S, steps)
        seen["per_instance" if per else "shared"] += 1
        seen["held"] += int(steps + 1 > T)
        seen["short_log"] += int(0 < S < steps)
        seen["no_log"] += int(S == 0)
        seen["bias"] += int(T == 1)
    assert all(v > 0 for v in seen.values()), seen


def test_reference_statement_on_known_cases():
    tab = np.arange(12.0).reshape(2, 3, 2)      # (B,T,nx)
    assert [MR.row_index(s, 3) for s in (-1, 0, 1, 2, 3, 99)] == [0, 0, 1, 2, 2, 2]
    assert np.array_equal(MR.rows(tab, 2, 7), [[4.0, 5.0], [10.0, 11.0]]) and np.array_equal(MR.rows(tab[0], 2, 1), [[2.0, 3.0], [2.0, 3.0]])
    assert np.array_equal(MR.measure(np.ones((2, 2)), tab, 0), [[1.0, 2.0], [7.0, 8.0]])
    X = np.zeros((2, 2, 4))
    assert np.array_equal(MR.measured_trajectory(X, tab)[:, :, 3], [[4.0, 5.0], [10.0, 11.0]])


def test_header_declares_the_entry_point_and_the_loader_binds_it():
    from robust_nonlinear_mpc_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slsqp.h")).read(), flags=re.S)
    mt = re.search(r"\bint\s+slsqp_cl_set_meas_noise\s*\(([^)]*)\)\s*;", src)
    assert mt, "slsqp_cl_set_meas_noise is not declared in include/slsqp.h"
    args = [a.strip() for a in mt.group(1).split(",")]
    assert args == ["slsqp_handle *h", "const double *Nm", "int T", "int per_instance", "int loc"]
    assert "slsqp_cl_set_meas_noise" in _lib.EXPORTS
    mt = re.search(r"lib\.slsqp_cl_set_meas_noise\.argtypes\s*=\s*\[([^\]]*)\]", inspect.getsource(_lib.load))
    assert mt and len(mt.group(1).split(",")) == 5


def test_python_streams_table_and_keywords_without_a_handle():
    from robust_nonlinear_mpc_amd import BatchedFastSLS, ClosedLoopMPC, disturbance_stream, get_model, meas_noise_table, measurement_stream, run_monte_carlo
    from robust_nonlinear_mpc_amd.monte_carlo import _run_slice
    rs = np.random.RandomState(3)
    assert np.array_equal(disturbance_stream(3, 4, 5), np.stack([2.0 * rs.rand(5) - 1.0 for _ in range(4)]))      # the seed's own stream: unchanged
    v = measurement_stream(3, 6, 5)
    assert v.shape == (6, 5) and np.all(np.abs(v) <= 1.0) and np.array_equal(v, measurement_stream(3, 6, 5))
    assert not np.array_equal(v[:4], disturbance_stream(3, 4, 5)) and not np.array_equal(v, measurement_stream(4, 6, 5))
    m = get_model("rocket")
    E0 = np.asarray(m.E, dtype=float)
    u = np.stack([measurement_stream(s, 3, m.nw) for s in range(2)])
    t = meas_noise_table(m, u, 0.5)
    assert t.shape == (2, 3, m.nx) and np.array_equal(t, 0.5 * (u @ E0.T)) and np.array_equal(meas_noise_table(m, u), u @ E0.T)
    assert np.all(np.abs(np.linalg.solve(E0, meas_noise_table(m, u[0]).T)) <= 1.0 + 1e-12)      # amp = 1: inside E[0]'s box
    for fn in (ClosedLoopMPC.__init__, run_monte_carlo, _run_slice):
        assert inspect.signature(fn).parameters["meas_noise"].default is None
    assert hasattr(BatchedFastSLS, "set_meas_noise") and hasattr(ClosedLoopMPC, "set_meas_noise")
    for ex in ("closed_loop.py", "rocket_closed_loop.py"):
        assert '"--meas-noise"' in open(os.path.join(ROOT, "examples", ex)).read()

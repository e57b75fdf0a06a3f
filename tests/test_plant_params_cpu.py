"""Plant parameters without a GPU: csrc/dynamics.hpp with the pointer parameter source (host instantiation through tests/dyn_host_params.cpp)
against the reference's own ode / ddyn with changed `params` (tests/golden/dyn_{quadrotor,rocket}_params.npz), the pendulum against the numpy
statement of tests/plant_params_helpers.py; a vector of the defaults against the constants' bits; pack_plant_params; and the setter's validation
routine in a stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import plant_params_helpers as H
from conftest import GOLDEN, ROOT

MID = {"pendulum": 0, "quadrotor": 1, "rocket": 2}


def _scale(v):
    return max(1.0, float(np.max(np.abs(v))))


@pytest.mark.parametrize("name", ["quadrotor", "rocket"])
def test_pointer_source_reproduces_the_reference_with_changed_params(name):
    """ode to rtol 1e-12 / atol 1e-12 x scale, ddyn to rtol 1e-12 / atol 1e-13 x scale: the tolerances of tests/test_dynamics_cpu.py."""
    g = np.load(os.path.join(GOLDEN, f"dyn_{name}_params.npz"))
    P, X, U = g["P"], g["X"], g["U"]
    assert P.shape[0] == 3 and np.isfinite(g["ode"]).all() and np.isfinite(g["ddyn"]).all()
    d = H.host_defaults(MID[name])
    assert np.all((P != d[None, :]).any(axis=0)), "every parameter is changed in at least one set"
    for s in range(3):
        for i in range(X.shape[0]):
            o = H.host_ode_p(MID[name], X[i], U[i], P[s])
            assert np.allclose(o, g["ode"][s, i], rtol=1e-12, atol=1e-12 * _scale(g["ode"][s, i])), (s, i)
            f = H.host_ddyn_p(MID[name], X[i], U[i], P[s])
            assert np.allclose(f, g["ddyn"][s, i], rtol=1e-12, atol=1e-13 * _scale(g["ddyn"][s, i])), (s, i)


@pytest.mark.parametrize("fixture", ["dyn_pendulum.npz", "dyn_pendulum_script.npz"])
def test_pendulum_helper_is_the_reference_at_default_parameters(fixture):
    g = np.load(os.path.join(GOLDEN, fixture))
    d = H.host_defaults(0)
    for i in range(g["X"].shape[0]):
        assert np.allclose(H.pendulum_ode(g["X"][i], g["U"][i], d), g["ode"][i], rtol=1e-12, atol=1e-12 * _scale(g["ode"][i]))
        assert np.allclose(H.pendulum_ddyn(g["X"][i], g["U"][i], d), g["ddyn"][i], rtol=1e-12, atol=1e-13 * _scale(g["ddyn"][i]))


def test_pointer_source_pendulum_against_the_helper():
    """Three parameter sets, every parameter changed by its own factor in 0.7 .. 1.4, at the points of dyn_pendulum_script.npz."""
    g = np.load(os.path.join(GOLDEN, "dyn_pendulum_script.npz"))
    d = H.host_defaults(0)
    F = np.array([[1.15, 0.70, 1.0, 1.02], [0.85, 1.0, 1.30, 0.97], [1.0, 1.40, 0.75, 1.05]])
    for s in range(3):
        p = d * F[s]
        for i in range(g["X"].shape[0]):
            ro, rd = H.pendulum_ode(g["X"][i], g["U"][i], p), H.pendulum_ddyn(g["X"][i], g["U"][i], p)
            assert np.allclose(H.host_ode_p(0, g["X"][i], g["U"][i], p), ro, rtol=1e-12, atol=1e-12 * _scale(ro)), (s, i)
            assert np.allclose(H.host_ddyn_p(0, g["X"][i], g["U"][i], p), rd, rtol=1e-12, atol=1e-13 * _scale(rd)), (s, i)
        assert max(np.abs(H.pendulum_ddyn(g["X"][i], g["U"][i], p) - g["ddyn"][i]).max() for i in range(g["X"].shape[0])) > 1e-6      # the parameters reach the values


@pytest.mark.parametrize("fixture", ["dyn_{}.npz", "dyn_{}_script.npz"])
@pytest.mark.parametrize("name", H.NAMES)
def test_defaults_through_the_pointer_are_the_bits_of_the_constants(name, fixture):
    g = np.load(os.path.join(GOLDEN, fixture.format(name)))
    mid = MID[name]
    d = H.host_defaults(mid)
    for i in range(g["X"].shape[0]):
        assert np.array_equal(H.host_ode_p(mid, g["X"][i], g["U"][i], d), H.host_ode_c(mid, g["X"][i], g["U"][i])), i
        assert np.array_equal(H.host_ddyn_p(mid, g["X"][i], g["U"][i], d), H.host_ddyn_c(mid, g["X"][i], g["U"][i])), i


@pytest.mark.parametrize("name", H.NAMES)
def test_python_table_matches_the_header(name):
    from robust_nonlinear_mpc_amd import plant_param_defaults, plant_param_names
    assert np.array_equal(plant_param_defaults(name), H.host_defaults(MID[name]))
    assert len(plant_param_names(name)) == len(plant_param_defaults(name)) == {"pendulum": 4, "quadrotor": 7, "rocket": 13}[name]
    if name != "pendulum":
        assert list(plant_param_names(name)) == [str(k) for k in np.load(os.path.join(GOLDEN, f"dyn_{name}_params.npz"))["names"]]


def test_pack_plant_params():
    from robust_nonlinear_mpc_amd import get_model, pack_plant_params, plant_param_defaults
    m = get_model("rocket")
    d = plant_param_defaults(m)
    B = 4
    P = pack_plant_params(m, B, {"mass": 1.3})
    assert P.shape == (13,) and P[0] == 1.3 and np.array_equal(P[1:], d[1:])
    mass = np.array([1.0, 1.1, 1.2, 1.3])
    P = pack_plant_params("rocket", B, {"mass": mass, "servo_angle_time_constant": 0.13})
    assert P.shape == (B, 13) and np.array_equal(P[:, 0], mass) and np.all(P[:, 7] == 0.13) and np.array_equal(P[:, 1:7], np.tile(d[1:7], (B, 1)))
    assert np.array_equal(pack_plant_params(m, B, d * 1.1), d * 1.1)
    M = np.tile(d, (B, 1)) * np.linspace(0.9, 1.1, B)[:, None]
    assert np.array_equal(pack_plant_params(m, B, M), M)
    assert np.array_equal(pack_plant_params(m, B, {}), d)
    with pytest.raises(ValueError, match="unknown"):
        pack_plant_params(m, B, {"weight": 1.0})
    with pytest.raises(ValueError):
        pack_plant_params(m, B, d[:-1])
    with pytest.raises(ValueError, match="rows"):
        pack_plant_params(m, B, np.tile(d, (B + 1, 1)))
    with pytest.raises(ValueError):
        pack_plant_params(m, B, {"mass": np.ones(B + 1)})
    with pytest.raises(ValueError):
        pack_plant_params(m, B, np.tile(d[:5], (B, 1)))
    assert pack_plant_params(get_model("pendulum"), 4, np.arange(1.0, 5.0)).shape == (4,)      # np = B = 4: a vector is the shared row


def test_validation_routine_under_sanitizers():
    """The setter's validation (csrc/plant_params.hpp, free of HIP calls) in a stand-alone program with its own main, built with
    -fsanitize=address,undefined: every entry NaN / infinite / zero / negative in turn, wrong np, buffers of exactly (np) and (B,np)."""
    exe = os.path.join(ROOT, "tests", "_build", "plant_params_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    # (the sanitizer runtimes linked statically: the program needs nothing from its environment)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-o", exe, os.path.join(ROOT, "tests", "plant_params_check_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "plant_params_check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

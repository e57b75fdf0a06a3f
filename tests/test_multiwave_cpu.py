"""The multi-wave QP path (solve_waves, csrc/slsqp_mw.hpp): its ABI surface and the numpy prototype of its block cyclic reduction.

The prototype (scripts/proto/cr_normal_eq.py) is the yardstick of the GPU tests (tests/test_gpu_multiwave.py), so it is held here against the
sequential block LDL' prototype and a dense solve on the normal equations of the corpus QPs (tests/qp_corpus.py) at three weightings: an
active-set round at the reference optimum's set, a late and a mid interior-point iteration.

Measured (relative residual |Y nu - b|inf / |b|inf in long double, one seeded right-hand side per system; worst over the QPs with a reference optimum):
    plant      weighting    sequential   cyclic     worst ratio per system
    pendulum   active-set   1.8e-05      4.2e-06    3.3          late-ipm 1.4e-07 / 2.5e-08 / 3.8    mid-ipm 3.4e-12 / 4.6e-12 / 4.1
    quadrotor  active-set   6.7e-11      8.1e-11    3.5          late-ipm 1.5e-10 / 2.1e-10 / 2.1    mid-ipm 1.4e-11 / 2.1e-11 / 2.8
    rocket     active-set   2.9e-09      2.8e-09    2.2          late-ipm 5.6e-10 / 6.2e-09 / 11.1   mid-ipm 2.2e-10 / 1.6e-09 / 7.1
(`python scripts/proto/cr_normal_eq.py` prints the table, with one stream of right-hand sides per plant; profiles/r06/README.md keeps it.  With this
module's right-hand sides the worst ratio is 6.1, rocket `scaled-10000`, late interior point.)
The cap of 10 x per system is the one the feature was specified with, and it is a regression guard for THIS module's seeded right-hand sides, not a
bound of the method: the ratio of two residuals that are both a few hundred roundings of a cond 1e9 system moves with the right-hand side, and the
script's own stream reaches 11.1 on the same rocket system (`scaled-10000`) where this module's gives 6.1.  What the method guarantees is a residual of
the order eps cond(D_i) per eliminated block, as the sequential recursion does; the corpus-wide worst residuals of the two are within a factor 11.
The block inverses are np.linalg.inv as it comes: averaged with their
transposes they lose the small residual D D^-1 - I of LAPACK's inverse, and the reduction's residual on the rocket grows to 24 - 39 x the sequential one.
"""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "proto"))

import cr_normal_eq as CR  # noqa: E402
import qp_corpus as QC  # noqa: E402

NEW = ("slsqp_set_solve_waves", "slsqp_get_solve_waves", "slsqp_ne_solve")


def test_abi_surface():
    from robust_nonlinear_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "slsqp.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS, name
    assert isinstance(_lib.HandleOpts.solve_waves, property)
    assert ctypes.sizeof(_lib.Opts) == 104 and ctypes.sizeof(_lib.HandleOpts) == 104


@functools.lru_cache(maxsize=None)
def _systems(plant):
    qps = QC.corpus(plant)
    return [(q, r) for q, r in zip(qps, (QC.reference(q) for q in qps)) if r is not None]


@pytest.mark.parametrize("horizon", [1, 2, 3, 5, 7, 20, 64])
def test_prototype_any_horizon(horizon):
    """random well-conditioned systems of every horizon shape the reduction distinguishes: the three solvers agree"""
    rng = np.random.default_rng(horizon)
    nx, nu = 5, 2
    A, B = 0.5 * rng.normal(size=(horizon, nx, nx)), rng.normal(size=(horizon, nx, nu))
    D, C = CR.stage_blocks(A, B, rng.uniform(0.1, 1.0, (nx + nu) * horizon + nx))
    b = rng.normal(size=(horizon, nx))
    x = np.linalg.solve(CR.dense(D, C), b.ravel()).reshape(horizon, nx)
    F, ok = CR.cr_factor(D, C)
    assert ok
    for nu_ in (CR.seq_solve(D, C, b), CR.cr_solve(F, b)):
        assert np.abs(nu_ - x).max() < 1e-12 * max(1.0, np.abs(x).max())
    b2 = rng.normal(size=(horizon, nx))          # the stored factors alone solve a second right-hand side
    assert CR.residual(D, C, b2, CR.cr_solve(F, b2)) < 1e-13


@pytest.mark.parametrize("weighting", CR.WEIGHTINGS)
@pytest.mark.parametrize("plant", QC.PLANTS)
def test_prototype_residuals(plant, weighting):
    rng = np.random.default_rng(1)
    worst = (0.0, None)
    for qp, ref in _systems(plant):
        D, C, _ = CR.system(qp, CR.active_mask(qp, ref), weighting)
        b = rng.normal(size=(qp.N, qp.nx))
        nu_c, ok = CR.cr(D, C, b)
        assert ok, (qp.name, "a block of the reduction is not positive definite")
        r_seq, r_cr = CR.residual(D, C, b, CR.seq_solve(D, C, b)), CR.residual(D, C, b, nu_c)
        nu_d = np.linalg.solve(CR.dense(D, C), b.ravel()).reshape(qp.N, qp.nx)
        r_d = CR.residual(D, C, b, nu_d)
        print(f"{plant} {weighting} {qp.name}: sequential {r_seq:.2e} cyclic {r_cr:.2e} dense {r_d:.2e} ratio {r_cr / r_seq:.1f}")
        # agreement with the dense solve: both are solutions of the same system to their residuals, so they differ by at most cond(Y) times those
        cond = np.linalg.cond(CR.dense(D, C))
        assert np.abs(nu_c - nu_d).max() <= 4.0 * cond * (r_cr + r_d) * np.abs(b).max() / np.abs(CR.dense(D, C)).sum(axis=1).max() + 1e-12 * np.abs(nu_d).max(), qp.name
        if r_cr / r_seq > worst[0]:
            worst = (r_cr / r_seq, qp.name)
    assert worst[0] <= 10.0, f"{plant} {weighting}: cyclic reduction {worst[0]:.1f} x the sequential residual on {worst[1]}"
